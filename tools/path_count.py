"""dev: issued instructions along a path of basic blocks of one kernel in a
gfx950 listing (hipcc -O3 -S --cuda-device-only with csrc/Makefile's flags).

  python tools/path_count.py file.s <kernel-substring>             lists the blocks
  python tools/path_count.py file.s <kernel-substring> A B C-1 ..  counts a path

A block is named by its label without the .LBB<fn>_ prefix (`531`) or, for an
unlabelled fall-through block, `bb.<N>`.  `C-1` drops the block's last
instruction (the branch after a taken conditional branch).  Every issued
instruction counts, s_nop and s_waitcnt included, by the first letter of its
mnemonic; register copies are v_mov_b32 / v_mov_b64 from a VGPR to a VGPR
outside inline asm."""
import collections
import re
import sys


def blocks(path, name):
    s = open(path).read()
    m = re.search(r"^(_Z\S*" + re.escape(name) + r"\S*):", s, re.M)
    body = s[m.end():s.index(".Lfunc_end", m.end())].splitlines()
    out, cur, in_asm = collections.OrderedDict(), None, False
    for l in body:
        t = l.strip()
        m1 = re.match(r"^\.LBB\d+_(\d+):", l)
        m2 = re.match(r"^; %bb\.(\d+):", l)
        if m1 or m2:
            cur = m1.group(1) if m1 else "bb." + m2.group(1)
            out[cur] = []
            continue
        if t.startswith(";;#ASMSTART"):
            in_asm = True
        elif t.startswith(";;#ASMEND"):
            in_asm = False
        if cur is None or not t or t.startswith((";", ".")):
            continue
        out[cur].append((t, in_asm))
    return out


def kind(t, in_asm):
    op = t.split()[0]
    if not in_asm and re.match(r"v_mov_b(32|64)(_e32)? v\[?\d+(:\d+\])?, v\[?\d+", t):
        return "vgpr_copy"
    return {"v": "valu", "s": "salu", "d": "ds"}.get(op[0], op)


if __name__ == "__main__":
    B = blocks(sys.argv[1], sys.argv[2])
    if len(sys.argv) == 3:
        for k, v in B.items():
            print(k, len(v), v[0][0] if v else "", "...", v[-1][0] if v else "")
        sys.exit(0)
    c = collections.Counter()
    for a in sys.argv[3:]:
        drop = a.endswith("-1")
        ins = B[a[:-2] if drop else a]
        for t, in_asm in (ins[:-1] if drop else ins):
            c[kind(t, in_asm)] += 1
            c["issued"] += 1
    c["valu"] += c["vgpr_copy"]  # (the copies are VALU moves: counted in both)
    print(dict(c))
