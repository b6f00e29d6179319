"""GPU tests of maximum_matching_sparse, check_matching_sparse and
maximum_bipartite_matching (the lsap_match_csr_ and lsap_check_hall_csr_
entries) against the host references of csr_hall_ref: card and the canonical
witness bit for bit, a valid match, the check's counts and flags on the
solver's own output and on tampered output, and card == nr_b exactly when the
cost solver finds an assignment."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import csr_hall_families as F  # noqa: E402
import csr_hall_ref as R  # noqa: E402
import lsap_sparse_families as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    for name in ("maximum_matching_sparse", "check_matching_sparse", "maximum_bipartite_matching"):
        assert hasattr(santa_hip, name), f"santa_hip has no {name}"
    return santa_hip


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def rows_of(indptr, nr, k):
    return indptr[k * nr:(k + 1) * nr + 1]


def reference(indptr, indices, data, nr, nc, B, shapes=None):
    out = [R.match_ref(rows_of(indptr, nr, k), indices, data, nr, nc, None if shapes is None else shapes[k])
           for k in range(B)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def check_reference(indptr, indices, data, nr, nc, match, wit, shapes=None):
    out = [R.check_ref(rows_of(indptr, nr, k), indices, data, nr, nc, match[k], wit[k],
                       None if shapes is None else shapes[k]) for k in range(match.shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def matched(sh, indptr, indices, data, nr, nc, B, shapes=None, dtype=torch.float64, **kw):
    match, card, wit = sh.maximum_matching_sparse(dev(indptr), dev(indices), dev(data, dtype), shape=(B, nr, nc),
                                                  shapes=shapes, **kw)
    assert match.dtype == torch.int32 and tuple(match.shape) == (B, nr)
    assert card.dtype == torch.int32 and tuple(card.shape) == (B,)
    assert wit.dtype == torch.uint8 and tuple(wit.shape) == (B, nr)
    return match.cpu().numpy(), card.cpu().numpy(), wit.cpu().numpy()


def checked(sh, indptr, indices, data, nr, nc, match, wit, shapes=None, **kw):
    B = match.shape[0]
    counts, fl = sh.check_matching_sparse(dev(indptr), dev(indices), dev(data), (B, nr, nc), dev(match), dev(wit),
                                          shapes=shapes, **kw)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, 3) and tuple(fl.shape) == (B,)
    return counts.cpu().numpy(), fl.cpu().numpy()


def assert_valid(indptr, indices, data, nr, nc, match, card, shapes=None):
    """match is a matching of the edges with card pairs, -1 in the padding."""
    for k in range(match.shape[0]):
        shape = None if shapes is None else shapes[k]
        nrb, ncb, kind = R.shape_kind(nr, nc, shape)
        E = R.edges(rows_of(indptr, nr, k), indices, data, nr, nc, shape)
        live = match[k, :nrb] if kind == "live" else match[k, :0]
        assert (match[k, live.size:] == -1).all(), k
        got = live[live >= 0]
        assert (live >= -1).all() and got.size == card[k] and np.unique(got).size == got.size, k
        assert E[np.flatnonzero(live >= 0), got].all(), (k, "a matched pair that is no edge")


@pytest.mark.parametrize("module,family,nr,nc", F.all_cases())
def test_matching_and_witness_equal_the_reference(sh, module, family, nr, nc):
    b = F.batch_of(module, family, nr, nc)
    B = len(b.dense)
    shapes = np.array(b.corners, dtype=np.int32) if b.corners else None
    data = b.data
    if shapes is not None:
        data = np.where(np.isnan(data), 1.0, data)  # (outside the corners: never an edge, but validate refuses NaN)
    match, card, wit = matched(sh, b.indptr, b.indices, data, nr, nc, B, shapes)
    want_card, want_wit = reference(b.indptr, b.indices, data, nr, nc, B, shapes)
    print("card", card.tolist(), "reference", want_card.tolist())
    assert np.array_equal(card, want_card) and np.array_equal(wit, want_wit)
    assert_valid(b.indptr, b.indices, data, nr, nc, match, card, shapes)
    counts, fl = checked(sh, b.indptr, b.indices, data, nr, nc, match, wit, shapes)
    want_counts, want_fl = check_reference(b.indptr, b.indices, data, nr, nc, match, wit, shapes)
    assert np.array_equal(counts, want_counts) and np.array_equal(fl, want_fl)
    for k in range(B):
        nrb, _, kind = R.shape_kind(nr, nc, None if shapes is None else shapes[k])
        nrb = nrb if kind == "live" else 0
        assert fl[k] == (0 if card[k] == nrb else R.DEFICIENT), (k, fl[k], counts[k])
        assert counts[k, 0] == card[k] and counts[k, 1] - counts[k, 2] == nrb - card[k]
    # float32 storage: the same edges
    m32, c32, w32 = matched(sh, b.indptr, b.indices, data, nr, nc, B, shapes, dtype=torch.float32)
    assert np.array_equal(c32, card) and np.array_equal(w32, wit)
    if module == S.__name__:  # the cost solver's own answer: an assignment exactly where card == nr_b
        col, _ = sh.solve_batched_sparse(dev(b.indptr), dev(b.indices), dev(data), shape=(B, nr, nc), shapes=shapes,
                                         with_cost=False)
        col = col.cpu().numpy()
        for k in range(B):
            r = b.dense[k].shape[0]
            assert (r > 0 and (col[k, :r] >= 0).all()) == (r > 0 and card[k] == r), k
            assert bool(b.feasible[k]) == (r > 0 and card[k] == r), k


@pytest.fixture(scope="module")
def deficient(sh):
    nr, nc = 40, 129
    b = F.batch("deficient_k", nr, nc)
    match, card, wit = matched(sh, b.indptr, b.indices, b.data, nr, nc, len(b.dense))
    assert (card < nr).all()
    return b, nr, nc, match, card, wit


def test_each_tampering_is_flagged_as_the_reference_says(sh, deficient):
    b, nr, nc, match, card, wit = deficient
    match, wit = match.copy(), wit.copy()
    E = [R.edges(rows_of(b.indptr, nr, k), b.indices, b.data, nr, nc) for k in range(8)]
    wit[0, np.flatnonzero(match[0, :nr] < 0)[0]] = 0           # one bit cleared (an unmatched row: N(R) stays)
    seen = E[1][wit[1] != 0].any(axis=0)
    wide = max(np.flatnonzero(wit[1] == 0), key=lambda i: int((E[1][i] & ~seen).sum()))
    assert (E[1][wide] & ~seen).sum() > 1
    wit[1, wide] = 1                                           # one set: two new columns or more
    i = int(np.flatnonzero(match[2] >= 0)[0])
    match[2, i] = int(np.flatnonzero(~E[2][i])[0])             # moved to a non-edge
    rows = np.flatnonzero(match[3] >= 0)
    match[3, rows[0]] = match[3, rows[1]]                      # moved to a taken column
    match[4, np.flatnonzero(match[4] < 0)[0]] = nc             # no column at all
    match[5, rows[0]] = -1                                     # a pair dropped: no longer maximum
    wit[6] = 0                                                 # no witness
    counts, fl = checked(sh, b.indptr, b.indices, b.data, nr, nc, match, wit)
    want_counts, want_fl = check_reference(b.indptr, b.indices, b.data, nr, nc, match, wit)
    print(counts.tolist(), fl.tolist(), want_fl.tolist())
    assert np.array_equal(counts, want_counts) and np.array_equal(fl, want_fl)
    assert fl[0] == R.WITNESS | R.DEFICIENT and fl[1] == R.WITNESS | R.DEFICIENT
    assert fl[2] & R.MATCH and fl[3] & R.MATCH and fl[4] & R.MATCH
    assert fl[5] == R.WITNESS | R.DEFICIENT and fl[6] == R.WITNESS | R.DEFICIENT and fl[7] == R.DEFICIENT
    # match and wit of other dtypes are the same claims
    c64, f64 = sh.check_matching_sparse(dev(b.indptr), dev(b.indices), dev(b.data), (8, nr, nc),
                                        dev(match.astype(np.int64)), dev(wit != 0))
    assert np.array_equal(c64.cpu().numpy(), counts) and np.array_equal(f64.cpu().numpy(), fl)


def test_a_feasible_matching_tampered(sh):
    nr, nc = 63, 65
    b = F.batch("chain_open", nr, nc)
    match, card, wit = matched(sh, b.indptr, b.indices, b.data, nr, nc, 8)
    assert (card == nr).all() and not wit.any()
    match, wit = match.copy(), wit.copy()
    wit[0, 5] = 1                                  # a row and its two columns: nR - nN == -1
    match[1, 10] = 64                              # a non-edge
    match[2, 10] = match[2, 11]                    # a taken column
    counts, fl = checked(sh, b.indptr, b.indices, b.data, nr, nc, match, wit)
    want_counts, want_fl = check_reference(b.indptr, b.indices, b.data, nr, nc, match, wit)
    assert np.array_equal(counts, want_counts) and np.array_equal(fl, want_fl)
    assert fl.tolist() == [R.WITNESS, R.MATCH, R.MATCH, 0, 0, 0, 0, 0]


def test_pattern_only_and_maximize(sh):
    nr, nc = 40, 129
    b = F.batch("inf_edges", nr, nc)
    B = len(b.dense)
    _, card, wit = matched(sh, b.indptr, b.indices, b.data, nr, nc, B)
    assert (card < nr).all()
    # values=None: every stored entry is an edge, and the stored pattern is feasible
    match, pcard, pwit = matched(sh, b.indptr, b.indices, None, nr, nc, B)
    want_card, want_wit = reference(b.indptr, b.indices, None, nr, nc, B)
    assert np.array_equal(pcard, want_card) and (pcard == nr).all() and not pwit.any()
    assert_valid(b.indptr, b.indices, None, nr, nc, match, pcard)
    counts, fl = checked(sh, b.indptr, b.indices, None, nr, nc, match, pwit)
    assert not fl.any() and (counts == np.array([nr, 0, 0])).all()
    # ... which the values refuse: the same claim is no matching of the edges
    counts, fl = checked(sh, b.indptr, b.indices, b.data, nr, nc, match, pwit)
    want_counts, want_fl = check_reference(b.indptr, b.indices, b.data, nr, nc, match, pwit)
    assert np.array_equal(counts, want_counts) and np.array_equal(fl, want_fl) and (fl & R.MATCH).all()
    # maximize: the forbidden value is -inf
    mmatch, mcard, mwit = matched(sh, b.indptr, b.indices, -b.data, nr, nc, B, maximize=True)
    assert np.array_equal(mcard, card) and np.array_equal(mwit, wit)
    counts, fl = checked(sh, b.indptr, b.indices, -b.data, nr, nc, mmatch, mwit, maximize=True)
    assert (fl == R.DEFICIENT).all()
    # one torch.sparse_csr tensor in place of the triple
    A = torch.sparse_csr_tensor(dev(b.indptr), dev(b.indices).long(), dev(b.data), size=(B * nr, nc))
    _, tcard, twit = sh.maximum_matching_sparse(A, shape=(B, nr, nc))
    assert np.array_equal(tcard.cpu().numpy(), card) and np.array_equal(twit.cpu().numpy(), wit)


def test_indices_outside_the_matrix_are_no_edges(sh, deficient):
    b, nr, nc, match, card, wit = deficient
    idx, val, ptr = [], [], [0]
    for r in range(8 * nr):
        e0, e1 = b.indptr[r], b.indptr[r + 1]
        idx += [-1 - r] + b.indices[e0:e1].tolist() + [nc, np.iinfo(np.int32).max]
        val += [1.0] + b.data[e0:e1].tolist() + [1.0, 1.0]
        ptr.append(len(idx))
    ptr, idx, val = np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int32), np.array(val)
    _, card2, wit2 = matched(sh, ptr, idx, val, nr, nc, 8, validate=False)
    assert np.array_equal(card2, card) and np.array_equal(wit2, wit)
    counts, fl = checked(sh, ptr, idx, val, nr, nc, match, wit)
    assert (fl == R.DEFICIENT).all()


@pytest.mark.parametrize("family,nr,nc", [("chain_closed", 65, 65), ("deficient_k", 129, 300), ("chain_open", 300, 300)])
def test_maximum_bipartite_matching_has_scipys_size(sh, family, nr, nc):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    g = F.FAMILIES[family](nr, nc, 2)
    A = csr_matrix((np.ones(g.data.size), g.indices, g.indptr), shape=(nr, nc))
    for M in (A, A.T.tocsr()):   # wide and tall
        want = maximum_bipartite_matching(M, perm_type="column")
        got = sh.maximum_bipartite_matching(M)
        assert got.dtype == np.int64 and got.shape == want.shape
        assert (got >= 0).sum() == (want >= 0).sum()
        rows = np.flatnonzero(got >= 0)
        assert np.unique(got[rows]).size == rows.size and np.asarray(M[rows, got[rows]]).all()
    t = sh.maximum_bipartite_matching((g.indptr, g.indices, g.data, (nr, nc)))
    assert (t >= 0).sum() == (want >= 0).sum()
