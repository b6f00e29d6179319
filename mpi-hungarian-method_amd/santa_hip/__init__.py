"""santa_hip — MI355X-native block-Hungarian optimiser for Kaggle Santa 2017.

A from-scratch gfx950 build of the hot path of bigzhao/MPI-Hungarian-method
(mpi_single.py / mpi_twins.py): block cost build + scipy-exact LSAP + swap
apply + score, behind the C-ABI in include/santa_hip.h (libsanta_hip.so).

Reference-surface entry points:
    init(child_data, gift_data)                 module set-up (tables -> HBM)
    avg_normalized_happiness(pred, child_pref, gift_pref)
    optimize_block(child_block, current_gift_ids)
    optimize_block_twins(child_block, subm)
    optimize_block_triplets(child_block, subm)   (extension: 3-slot triplet units)
    linear_sum_assignment(C)
    my_optimizer(subm, score_org, comm, rank, size, gift_data, child_data)
"""
from ._lib import LIB_PATH, SantaHipError, lib  # noqa: F401  (fails loudly if the .so is missing)
from .api import (avg_normalized_happiness, init, optimize_block,  # noqa: F401
                  optimize_block_triplets, optimize_block_twins, session)
from .context import SantaGPU, score_from_sums  # noqa: F401
from .driver import my_optimizer, run_rounds  # noqa: F401
from ._lib import (SH_CERT_COL, SH_CERT_GAP, SH_CERT_NONE, SH_CERT_RANGE, SH_CERT_SIGN,  # noqa: F401
                   SH_CERT_SLACK, SH_CERT_TIGHT, SH_HALL_DEFICIENT, SH_HALL_MATCH, SH_HALL_WITNESS)
from .lsap import (check_duals, check_duals_large, check_duals_sparse, check_matching_sparse,  # noqa: F401
                   csr_transpose, densify, maximum_bipartite_matching, maximum_matching_sparse,
                   linear_sum_assignment, linear_sum_assignment_duals, linear_sum_assignment_large,
                   linear_sum_assignment_resolve, linear_sum_assignment_sparse,
                   linear_sum_assignment_sparse_resolve, resolve_batched, resolve_batched_free_rows,
                   resolve_batched_sparse, resolve_batched_sparse_free_rows,
                   kbest_assignments, kbest_batched, murty_children_batched,
                   kbest_assignments_sparse, kbest_batched_sparse, murty_children_batched_sparse,
                   solve_batched, solve_batched_large, solve_batched_sparse, solve_hash, validate_csr)
from .lbap import check_bottleneck, linear_bottleneck_assignment, solve_bottleneck_batched  # noqa: F401

lib()  # load the C-ABI at import: no silent CPU path

__all__ = [
    "init", "session", "avg_normalized_happiness", "optimize_block", "optimize_block_twins",
    "optimize_block_triplets",
    "linear_sum_assignment", "linear_sum_assignment_duals", "solve_batched", "check_duals", "solve_hash",
    "linear_sum_assignment_large", "solve_batched_large", "check_duals_large",
    "linear_sum_assignment_resolve", "resolve_batched", "resolve_batched_free_rows",
    "linear_sum_assignment_sparse", "solve_batched_sparse", "densify", "csr_transpose", "validate_csr",
    "resolve_batched_sparse", "resolve_batched_sparse_free_rows", "linear_sum_assignment_sparse_resolve",
    "kbest_assignments", "kbest_batched", "murty_children_batched",
    "kbest_assignments_sparse", "kbest_batched_sparse", "murty_children_batched_sparse",
    "check_duals_sparse", "maximum_matching_sparse", "check_matching_sparse", "maximum_bipartite_matching",
    "linear_bottleneck_assignment", "solve_bottleneck_batched", "check_bottleneck",
    "SH_CERT_COL", "SH_CERT_SLACK", "SH_CERT_TIGHT", "SH_CERT_SIGN", "SH_CERT_GAP", "SH_CERT_NONE",
    "SH_CERT_RANGE", "SH_HALL_MATCH", "SH_HALL_WITNESS", "SH_HALL_DEFICIENT", "my_optimizer", "run_rounds",
    "SantaGPU", "score_from_sums", "SantaHipError",
]
