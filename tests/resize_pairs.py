"""What the resample pair sweeps share (tests/test_resize_pairs_host.py, tests/test_gpu_resize_pairs.py): sets of axis pairs
(n_in, n_out) at the smallest sizes where the structure build_taps_host derives from a tap table (csrc/resize.cpp: the regular
run, the up-sampling classes of up_axis_build, the records of down2_build) and the split plan_resample makes of a launch (bands,
strips, border tiles, job orders) can still go wrong, and the 2-D cases built from them.  Nothing here is drawn at random: the
same lists on every machine, so the host census and the device sweep speak about the same cases.

The sets:
  A  every pair with 1 <= n_in, n_out <= 24 (576 pairs);
  B  whole ratios and their neighbours: (i, R i + d) up and (R i + d, i) down for i in B_I, R in B_R, d in -1, 0, 1;
  C  outputs on quad, tile and strip edges (63 .. 257 columns) from sources an eighth to eight times as long;
  D  both axes structured: 32 down-sampling pairs crossed with themselves, and 64 up-sampling pairs with four partners each.

The cases (vertical pair, horizontal pair), the same for every filter; the plane count alternates 1, 4 by case index:
  * A with A by the permutation k -> (A_MUL k + A_ADD) mod 576: every A pair is a vertical table once and a horizontal one once;
  * every pair of B or C outside A twice: as the vertical table beside an A pair of its own direction (both axes up or both
    down: the forms that need two structured axes), and as the horizontal table beside any A pair;
  * D as described.
No source is larger than about 2056 x 24 (a B or C pair beside an A pair) or 265 x 265 (D).

Sources hold values in [-0.25, 1.25) with edge values on the first and last row, the first and last column and the last partial
(or whole) quad of columns.  At these sizes a down-sampling window covers much of the source, and one NaN in a corner would turn
most of the result into NaN; so only every other plane carries the non-finite values and the 3e38 pairs (util.SALT_VALUES), the
others the finite ones that leave the arithmetic visible (FINITE_SALT): in a 4-plane case planes 0 and 2 are the harsh ones, and
of the 1-plane cases every other one."""
import numpy as np

from util import SALT_VALUES, SEED_A, SEED_B, resize_source, salt

FILTERS = ["Nearest", "Triangle", "CatmullRom", "Gaussian", "Lanczos3"]
FINITE_SALT = [-0.0, 1e-40, 1.25, -0.25]

B_I = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 22, 23, 25, 32, 33]
B_R = [2, 3, 4, 5, 6, 7, 8, 12, 16]
C_OUT = [63, 64, 65, 127, 128, 129, 255, 256, 257]
A_MUL, A_ADD = 175, 101          # 175 = 5^2 7 is coprime to 576 = 2^6 3^2
SAME_MUL, SAME_ADD = 67, 5       # 67 is coprime to 276 = 2^2 3 23, the number of A pairs of one direction
ANY_MUL, ANY_ADD = 245, 17       # 245 = 5 7^2 is coprime to 576
# partners of the up-sampling D pair j: D_UP[(13 j + DU_ADD[t]) mod 64], t = 0 .. 3.  D_UP alternates whole ratios (even places)
# and their neighbours; two even and two odd offsets, the even ones at an even and an odd t, so that a whole ratio meets a whole
# ratio -- what the integer-ratio kernels need on both axes -- in a 1-plane case and in a 4-plane case
DU_MUL, DU_ADD = 13, (8, 22, 29, 51)


def _unique(pairs):
    seen, out = set(), []
    for p in pairs:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def set_a():
    return [(i, o) for i in range(1, 25) for o in range(1, 25)]


def set_b():
    out = []
    for i in B_I:
        for r in B_R:
            for d in (-1, 0, 1):
                if r * i + d >= 1:
                    out += [(i, r * i + d), (r * i + d, i)]
    return _unique(out)


def set_c():
    return _unique([(n, o) for o in C_OUT for n in (o // 8, o // 4, o // 2, o - 1, o + 1, 2 * o, 2 * o + 1, 4 * o, 8 * o)])


def set_d_down():
    return [(r * i + d, i) for i in (22, 23, 25, 33) for r in (2, 3, 4, 8) for d in (0, 1)]


def set_d_up():
    return [(i, r * i + d) for i in (1, 2, 3, 5, 8, 9, 16, 17) for r in (2, 4, 8, 12) for d in (0, 1)]


A, B, C, D_DOWN, D_UP = set_a(), set_b(), set_c(), set_d_down(), set_d_up()
ABC = _unique(A + B + C)          # the pairs the host tests sweep, and the device sweep in both roles
EXTRA = ABC[len(A):]              # the B and C pairs outside A


class Case:
    """One 2-D resample: .v, .h the vertical and horizontal pair, .kind the set it comes from ("A", "BC", "D_down", "D_up"),
    .index its place in CASES, .planes 1 or 4; .src and .dst are (width, height)."""

    def __init__(self, index, kind, v, h):
        self.index, self.kind, self.v, self.h = index, kind, v, h
        self.planes = 4 if index % 2 else 1
        self.src, self.dst = (h[0], v[0]), (h[1], v[1])

    def __repr__(self):
        return "case %d (%s): vertical %d->%d, horizontal %d->%d, %d plane%s" % (
            self.index, self.kind, self.v[0], self.v[1], self.h[0], self.h[1], self.planes, "s" if self.planes > 1 else "")


def _cases():
    out = []

    def add(kind, v, h):
        out.append(Case(len(out), kind, v, h))
    for k, v in enumerate(A):
        add("A", v, A[(A_MUL * k + A_ADD) % len(A)])
    same = {True: [p for p in A if p[0] < p[1]], False: [p for p in A if p[0] > p[1]]}
    for j, p in enumerate(EXTRA):
        mates = same[p[0] < p[1]]
        add("BC", p, mates[(SAME_MUL * j + SAME_ADD) % len(mates)])
        add("BC", A[(ANY_MUL * j + ANY_ADD) % len(A)], p)
    for v in D_DOWN:
        for h in D_DOWN:
            add("D_down", v, h)
    for j, v in enumerate(D_UP):
        for t in range(4):
            add("D_up", v, D_UP[(DU_MUL * j + DU_ADD[t]) % len(D_UP)])
    return out


CASES = _cases()
D_CASES = [c for c in CASES if c.kind.startswith("D")]
FUSED_CASES = [c for c in CASES if c.kind in ("A", "D_up")]
FUSED_FILTERS = ["Nearest", "Triangle"]

# The option modes of the device sweep: (id, {option: value}).  The first four run every case, the others the D cases.
MODES_ALL = [("default", {}), ("mode2", {"resize_mode": 2}), ("mode3", {"resize_mode": 3}), ("mode4", {"resize_mode": 4})]
MODES_D = [("mode1", {"resize_mode": 1}), ("down2_0", {"down2": 0}), ("down2_2", {"down2": 2}), ("poly2_min_ratio_2", {"poly2_min_ratio": 2}),
           ("poly_rows_4", {"poly_rows": 4}), ("down2_by_rows_0", {"down2_by_rows": 0}), ("down2_by_rows_1", {"down2_by_rows": 1}),
           ("down2_xcd_1", {"down2_xcd": 1}), ("poly2_xcd_0", {"poly2_xcd": 0}), ("poly2_xcd_2", {"poly2_xcd": 2}),
           ("tile_16x4", {"resize_tile_w": 16, "resize_tile_h": 4}), ("budget_0", {"cache_budget_mb": 0})]


def tables(cases=CASES, filters=FILTERS):
    """The distinct (n_in, n_out, filter) tap tables the cases need."""
    return {(p[0], p[1], f) for c in cases for p in (c.v, c.h) for f in filters}


def edge_columns(w):
    return [0, w - 1] + [w - 1 - k for k in range(w % 4 or 4)]


def harsh(case, plane):
    """Does this plane of the case carry the non-finite edge values (module docstring)?"""
    return plane % 2 == 0 if case.planes == 4 else (case.index // 2) % 2 == 0


def sources(case, seed=SEED_A, size=None):
    """The case's source planes (size: another (width, height), for the full-size operand of the fused cases)."""
    w, h = size or case.src
    return [salt(resize_source(seed + case.index, c, h, w), [0, h - 1], edge_columns(w), shift=c + case.index,
                 values=SALT_VALUES if harsh(case, c) else FINITE_SALT) for c in range(case.planes)]


def bases(case):
    """The full-size left operands of the fused cases: mix_process(base, resize_image(small, size, filter), Add)."""
    return sources(case, SEED_B, case.dst)


def first_difference(got, want):
    """(y, x, got bits, want bits) of the first sample that is not bit-equal (any NaN equals any NaN), or None."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if g.shape != w.shape:
        return (-1, -1, g.shape, w.shape)
    bad = ~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))
    if not bad.any():
        return None
    y, x = (int(v) for v in np.argwhere(bad)[0])
    return y, x, "0x%08x" % int(g.view(np.uint32)[y, x]), "0x%08x" % int(w.view(np.uint32)[y, x])
