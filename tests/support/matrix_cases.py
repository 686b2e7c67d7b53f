"""matrix_cases.py -- TEST INFRASTRUCTURE of the (type, op) pair matrix
(tests/test_matrix_ref.py, tests/test_gpu_pair_matrix.py): every pair of the
library through the shifted combine, the scan kernel, the uniform kernel and
the six collective front doors.

Nothing here folds.  Expected values are the case modules' (rscatter_cases,
scan_cases, uniform_cases, many_cases, loc_cases), i.e. the reduce-to-all
oracle's, or half_ref.fold for the 16-bit types.  This module adds

  * matrix_inputs: inputs laid out by POSITION so that every pair meets, at
    every length of a whole tile or more, the conditions conditions() measures
    with the oracle alone (tests/test_matrix_ref.py asserts them);
  * the lengths n_small / n_tile per kernel;
  * DoorCase / run_door: one collective call of a door on a cached Team.

The layout of a floating sum / prod input, by 16-byte vector v of the array
(k = v // 16 numbers the periods, one element of the vector is special, the
others ordinary):
  v % 4 == 1    payload NaNs in member 0 AND member 1, distinct: the ascending
                fold keeps member 0's, member 1's caller-first fold its own --
                the order-sensitive elements (a + b and a * b commute, so a
                fold that starts at the wrong member differs only here)
  v % 16 == 3   a payload NaN in a middle member (the second operand's NaN)
  v % 16 == 7   +inf then -inf (sum), 0 then inf (prod): the default NaN
  v % 16 == 11  complex prod: (inf + i NaN) at a middle member, the members
                after it real -- libgcc's recovery runs and the value ends as
                infinities; other pairs: a signalling NaN in a middle member
                and another NaN in the last
  v % 16 == 15  complex prod: (inf + i NaN) at member P - 2, the last member
                ordinary -- the recovery runs and a NaN part remains; other
                pairs: -inf then +inf, inf then 0
  even v        ordinary values: no NaN part, the branch-free fold's result
So half of the vectors keep the fast route and a quarter to a half take the
exact one, mixed inside every group of 64.
"""
from __future__ import annotations

import numpy as np

import oracle as O
from support import half_ref as R
from support import loc_cases as L
from support import many_cases as M
from support import rscatter_cases as C
from support import scan_cases as S
from support import uniform_cases as U

TYPES = O.TYPES + list(R.TYPES)
FLOATING = ("float", "double", "complexf", "complexd", "half", "bfloat16")   # the Fast<> types


def ops_of(t: str):
    if t in R.TYPES:
        return list(R.OPS)
    return [op for op in O.OPS if O.has_op(t, op)]


ALL_PAIRS = [(t, op) for t in TYPES for op in ops_of(t)]
assert len(ALL_PAIRS) == 52

DOORS = ("rscatter", "many", "scan_inc", "scan_exc", "uniform", "loc")
RAW_KERNELS = ("combine_shifted", "team_scan", "team_uniform")
# team_scan refuses long double (OSGPU_ENOTSUP): osgpu_scan serves it by the pull form
RAW_TYPES = {"combine_shifted": TYPES, "team_scan": [t for t in TYPES if t != "longdouble"],
             "team_uniform": TYPES}
MEMBERS = (2, 3, 8)
# the heaviest instantiations at 8 members on the collective (scan, uniform)
P8_PAIRS = [("complexd", "prod"), ("complexd", "sum"), ("double", "prod"), ("bfloat16", "prod"),
            ("half", "max"), ("longlong", "and")]


def door_pairs(door: str):
    return list(L.PAIRS) if door == "loc" else list(ALL_PAIRS)


def door_types(door: str):
    return list(L.TYPES) if door == "loc" else list(TYPES)


def raw_pairs(kernel: str):
    return [(t, op) for t in RAW_TYPES[kernel] for op in ops_of(t)]


esize, dtype, same_bits = C.esize, C.dtype, C.same_bits


def width(t: str) -> int:
    """W: elements per 16-byte vector."""
    return 16 // esize(t)


# ---------------------------------------------------------------- lengths
_DOOR_KERNEL = {"rscatter": "combine_shifted", "many": "combine_many", "scan_inc": "team_scan",
                "scan_exc": "team_scan", "uniform": "team_uniform", "loc": "team_loc"}


def tile_elems(kernel: str, t: str, P: int) -> int:
    """One tile of `kernel` in elements (per member), from the case modules."""
    if kernel == "team_loc":
        return L.tile_elems(t)
    if kernel == "team_uniform":
        return U.tile_elems(t, P)
    v = {"combine_shifted": C.TILE_VECTORS, "combine_many": M.TILE_VECTORS,
         "team_scan": S.TILE_VECTORS}[kernel]
    return v * width(t)


def n_small(t: str) -> int:
    """W + 1: one vector and a tail element (a head and a tail off phase 0)."""
    return width(t) + 1


def n_tile(kernel: str, t: str, P: int) -> int:
    """A whole tile, one more vector, W - 1 more elements: the smallest length
    with a head, a whole tile, a partial tile and a tail."""
    return tile_elems(kernel, t, P) + 2 * width(t) - 1


def n_collective(door: str, t: str, P: int = 3) -> int:
    """n_tile of the door's kernel, raised so that n * size > 4096 and is no
    multiple of 2048: GETMEM with a 2048-byte chunk walks at least two chunks
    and the last is ragged."""
    n = max(n_tile(_DOOR_KERNEL[door], t, P), 4096 // esize(t) + 1)
    if (n * esize(t)) % 2048 == 0:
        n += 1
    return n


# ----------------------------------------------------------------- inputs
# component formats: (unsigned view, four payload NaNs -- quiet, signalling,
# negative signalling, quiet -- distinct after quieting, +inf, sign bit)
_FMT = {
    "half": (np.uint16, (0x7E15, 0x7C01, 0xFD05, 0x7F23), 0x7C00, 0x8000),
    "bfloat16": (np.uint16, (0x7FD5, 0x7F81, 0xFFA5, 0x7FE3), 0x7F80, 0x8000),
    "f32": (np.uint32, (0x7FC00123, 0x7F800001, 0xFFA00005, 0x7FE00077), 0x7F800000, 0x80000000),
    "f64": (np.uint64, (0x7FF8000000000123, 0x7FF0000000000001, 0xFFF4000000000005,
                        0x7FFC000000000077), 0x7FF0000000000000, 0x8000000000000000),
}
_COMP = {"float": ("f32", 1), "complexf": ("f32", 2), "double": ("f64", 1), "complexd": ("f64", 2),
         "half": ("half", 1), "bfloat16": ("bfloat16", 1)}
# ordinary 16-bit values: sums that depend on the fold's rounding and stay
# finite over 8 members; factors round 1 whose products stay normal
_POOL16 = {
    ("half", "sum"): [0x3C00, 0x1000, 0x1001, 0x9000, 0x6BFF, 0xEBFF, 0x0001, 0x83FF, 0x3C01,
                      0x4248, 0xB555, 0x0000, 0x8000, 0x5640],
    ("half", "prod"): [0x3C00, 0x3C01, 0x3C03, 0x3BFF, 0x4000, 0x3800, 0xBC01, 0x3E00, 0x3555,
                       0xB801, 0x3C7F, 0x4100],
    ("bfloat16", "sum"): [0x3F80, 0x3B80, 0x3B81, 0xBB80, 0x4B7F, 0xCB7F, 0x0001, 0x807F, 0x3F81,
                          0x4049, 0xBEAB, 0x0000, 0x8000, 0x42C8],
    ("bfloat16", "prod"): [0x3F80, 0x3F81, 0x3F83, 0x3F7F, 0x4000, 0x3F00, 0xBF81, 0x3FC0, 0x3EAB,
                           0xBF01, 0x3F8F, 0x4020],
}


def _ordinary(t: str, op: str, n: int, seed: int) -> np.ndarray:
    """n finite values without specials (no NaN, no infinity)."""
    if t in R.TYPES:
        arith = op if op in ("sum", "prod") else "sum"
        pool = np.array(_POOL16[(t, arith)], np.uint16)
        return pool[np.random.default_rng(seed).integers(0, pool.size, n)]
    return O.gen_input(t, n, seed, "prod" if op == "prod" else "mixed")


def _view(t: str, a: np.ndarray) -> np.ndarray:
    """The (n, components) unsigned view of an array of a _COMP type."""
    fmt, comps = _COMP[t]
    return a.view(_FMT[fmt][0]).reshape(-1, comps)


def _arith_inputs(t: str, op: str, P: int, n: int, seed: int):
    """Floating sum / prod: the layout of the module docstring."""
    fmt, comps = _COMP[t]
    _, nans, inf, sign = _FMT[fmt]
    W = width(t)
    out = [np.array(_ordinary(t, op, n, O.pe_seed(seed, p)), copy=True) for p in range(P)]
    u = [_view(t, a) for a in out]
    cplx_prod = comps == 2 and op == "prod"
    mid = max(P - 2, 1)
    for v in range(1, (n + W - 1) // W, 2):
        k = v // 16
        e = min(v * W + k % W, n - 1)
        c = (v // 4) % comps
        j = min(1 + k % mid, P - 1)          # a middle member (the last of two)
        a = k % (P - 1)                      # the first of two adjacent members
        cls = v % 16
        if v % 4 == 1:
            u[0][e, c] = nans[(k + cls // 4) % 4]
            u[1][e, c] = nans[(k + cls // 4 + 1) % 4]
        elif cls == 3:
            u[j][e, c] = nans[k % 4]
        elif cls == 7 or (cls == 15 and not cplx_prod):
            first, second = (inf, inf | sign) if op == "sum" else ((k % 2) * sign, inf)
            if cls == 15:
                first, second = second, first
            if cplx_prod:                    # (0, 0) then (inf, ordinary): 0 * inf in both parts
                u[a][e, :] = first
                u[a + 1][e, 0] = second
            else:
                u[a][e, c], u[a + 1][e, c] = first, second
        elif cls == 11 and cplx_prod:
            u[j][e, 0], u[j][e, 1] = inf, nans[k % 4]
            for q in range(j + 1, P):
                u[q][e, 1] = (q % 2) * sign  # real factors: the recovery gives infinities again
        elif cls == 11:
            u[j][e, c] = nans[1 + k % 2]
            u[P - 1][e, c] = nans[(k + 3) % 4]
        elif cls == 15:                      # complex prod: the recovery, then an ordinary factor
            u[max(P - 2, 0)][e, 0], u[max(P - 2, 0)][e, 1] = inf, nans[(k + 2) % 4]
    return out


def _one(t: str):
    return np.array([1], dtype(t)) if t not in R.TYPES else \
        np.array([0x3C00 if t == "half" else 0x3F80], np.uint16)


def _extreme_inputs(t: str, op: str, P: int, n: int, seed: int):
    """max / min of a floating type (long double apart): by element i,
    i % 4 == 1 a tie of all members; i % 16 == 0 / 2 / 3 a payload NaN in the
    first / a middle / the last member; 4 / 6 signed zeros alternating from +0
    / from -0; 7 / 8 all -inf / all +inf; 10 draws of loc_cases.alphabet;
    the others ordinary."""
    fmt, _ = _COMP[t]
    ut, nans, inf, sign = _FMT[fmt]
    out = [np.array(_ordinary(t, op, n, O.pe_seed(seed, p)), copy=True) for p in range(P)]
    u = [a.view(ut) for a in out]
    rng = np.random.default_rng(seed ^ 0xA1FA)
    alpha = L.alphabet(t).view(ut)
    i = np.arange(n)
    k = i // 16
    for p in range(P):
        u[p][i % 16 == 4] = (p % 2) * sign
        u[p][i % 16 == 6] = ((p + 1) % 2) * sign
        u[p][i % 16 == 7] = inf | sign
        u[p][i % 16 == 8] = inf
        m = i % 16 == 10
        u[p][m] = alpha[rng.integers(0, alpha.size, int(m.sum()))]
        if p:
            u[p][i % 4 == 1] = u[0][i % 4 == 1]
    mid = max(P - 2, 1)
    for cls, member in ((0, np.zeros(n, int)), (2, np.minimum(1 + k % mid, P - 1)),
                        (3, np.full(n, P - 1))):
        for p in range(P):
            m = (i % 16 == cls) & (member == p)
            u[p][m] = np.array(nans, ut)[k[m] % 4]
    return out


def _int_inputs(t: str, op: str, P: int, n: int, seed: int):
    """Integers: raw bits with the type's minimum and maximum at i % 16 == 0 /
    2 in one member; prod small factors, with large ones (a product that
    wraps) at i % 8 == 3; max / min a tie of all members at i % 4 == 1."""
    out = [np.array(a, copy=True) for a in O.team_inputs(t, P, n, seed, "prod" if op == "prod" else "bits")]
    ii = np.iinfo(dtype(t))
    i = np.arange(n)
    for p in range(P):
        mine = (i // 16) % P == p
        out[p][(i % 16 == 0) & mine] = ii.min
        out[p][(i % 16 == 2) & mine] = ii.max
        if op == "prod":
            out[p][i % 8 == 3] = (ii.max // 3) - 7 * p
        if op in ("max", "min") and p:
            out[p][i % 4 == 1] = out[0][i % 4 == 1]
    return out


def _longdouble_inputs(op: str, P: int, n: int, seed: int):
    """The oracle's edge set (NaNs with payloads, signed zeros, the x87
    encodings with no IEEE counterpart) in every second element -- one edge row
    per member and element, the rows walked so that every row meets every other
    -- over the mixed values; max / min a tie of all members at i % 4 == 1."""
    sv = O.special_values("longdouble")
    out = [np.array(a, copy=True) for a in O.team_inputs("longdouble", P, n, seed, "prod" if op == "prod" else "mixed")]
    i = np.arange(n)
    for p in range(P):
        m = i % 2 == 0
        out[p][m] = sv[(i[m] // 2 * (p + 1) + 5 * p) % sv.size]
        if op in ("max", "min") and p:
            out[p][i % 4 == 1] = out[0][i % 4 == 1]
    return out


def matrix_inputs(t: str, op: str, P: int, n: int, seed: int):
    """P arrays of n elements (uint16 patterns for the 16-bit types) meeting
    conditions(t, op, ...) at P >= 3 and n of a whole tile or more."""
    if n == 0:
        return [np.zeros(0, dtype(t)) for _ in range(P)]
    if t in O.INT_TYPES:
        return _int_inputs(t, op, P, n, seed)
    if t == "longdouble":
        return _longdouble_inputs(op, P, n, seed)
    if op in ("sum", "prod"):
        return _arith_inputs(t, op, P, n, seed)
    return _extreme_inputs(t, op, P, n, seed)


# ------------------------------------------- the conditions, by the oracle
def has_nan(t: str, a) -> np.ndarray:
    """Per element: some part is a NaN."""
    if t in R.TYPES:
        return R.isnan(t, a)
    a = np.asarray(a)
    if t in O.CPLX:
        return np.isnan(a.real) | np.isnan(a.imag)
    return np.isnan(a) if t in O.REAL_FP else np.zeros(a.shape, bool)


def _steps(t: str, op: str, srcs):
    """The ascending fold's running values [after member 0, after member 1, ...]
    (the scan's inclusive results: the oracle over sub-sets)."""
    return S.inclusive(t, op, list(srcs))


def _by_vector(flag: np.ndarray, W: int, head: int = 0) -> np.ndarray:
    """Per 16-byte vector of an array whose first `head` elements are a scalar
    head: any element flagged (the tail's partial vector is left out)."""
    body = flag[head:]
    nv = body.size // W
    return body[:nv * W].reshape(nv, W).any(axis=1)


def conditions(t: str, op: str, srcs) -> dict:
    """What the oracle alone says about the inputs `srcs` (P arrays) of (t, op):
    the figures tests/test_matrix_ref.py holds against the issue's thresholds."""
    P, n = len(srcs), len(srcs[0])
    W = width(t)
    out = {}
    if t in FLOATING and op in ("sum", "prod"):
        inc = _steps(t, op, srcs)
        final = inc[-1]
        nan_in = [has_nan(t, s) for s in srcs]
        any_in = np.logical_or.reduce(nan_in)
        nan_out = has_nan(t, final)
        for head in (0, 1 % W):
            vec_nan = _by_vector(nan_out, W, head)
            # the fast route is kept where no running value has a NaN part
            vec_exact = _by_vector(np.logical_or.reduce([has_nan(t, x) for x in inc]) | any_in, W, head)
            out[f"vectors_h{head}"] = vec_nan.size
            out[f"fast_vectors_h{head}"] = int((~vec_exact).sum())
            out[f"nan_vectors_h{head}"] = int(vec_nan.sum())
            g = vec_nan.size // 64 * 64
            both = [vec_nan[i:i + 64].any() and not vec_exact[i:i + 64].all()
                    for i in range(0, max(g, 1), 64)]
            out[f"mixed_groups_h{head}"] = int(sum(both))
        out["nan_from_first"] = int((nan_in[0] & nan_out).sum())
        out["nan_from_middle"] = int(np.logical_or.reduce(
            [nan_in[j] & ~np.logical_or.reduce(nan_in[:j]) for j in range(1, max(P - 1, 2))]).sum())
        out["nan_from_arithmetic"] = int((nan_out & ~any_in).sum())
        # a fold that starts at member 1 (its caller-first order) differs here
        other = C.to_all(t, op, list(srcs))[1] if t in R.TYPES else O.to_all(t, op, list(srcs))[1]
        fb = np.ascontiguousarray(final).view(np.uint8).reshape(n, -1)
        ob = np.ascontiguousarray(other).view(np.uint8).reshape(n, -1)
        out["order_sensitive"] = int((fb != ob).any(axis=1).sum())
        if t in O.CPLX and op == "prod":
            ran = np.zeros(n, bool)
            comp = np.float32 if t == "complexf" else np.float64
            for j in range(1, P):
                a, b = inc[j - 1], np.asarray(srcs[j])
                with np.errstate(all="ignore"):
                    x = (a.real * b.real).astype(comp) - (a.imag * b.imag).astype(comp)
                    y = (a.real * b.imag).astype(comp) + (a.imag * b.real).astype(comp)
                step = inc[j]
                recovered = np.isnan(x) & np.isnan(y) & ~(np.isnan(step.real) & np.isnan(step.imag))
                if 1 <= j <= max(P - 2, 1):
                    ran |= recovered
            out["recovered_clean"] = int((ran & ~nan_out).sum())
            out["recovered_nan"] = int((ran & nan_out).sum())
    if op in ("max", "min") and (t in FLOATING or t == "longdouble"):
        nan_in = [has_nan(t, s) for s in srcs]
        out["nan_first"] = int(nan_in[0].sum())
        out["nan_middle"] = int(np.logical_or.reduce(nan_in[1:max(P - 1, 2)]).sum())
        out["nan_last"] = int(nan_in[P - 1].sum())
        if t != "longdouble":
            f = np.stack([L.numeric(t, s) for s in srcs])
            neg = np.stack([np.signbit(L.numeric(t, s)) for s in srcs])
            zero = (f == 0).all(axis=0)
            out["zeros_plus_first"] = int((zero & ~neg[0] & neg[1:].any(axis=0)).sum())
            out["zeros_minus_first"] = int((zero & neg[0] & (~neg[1:]).any(axis=0)).sum())
            out["all_minus_inf"] = int((f == -np.inf).all(axis=0).sum())
            out["all_plus_inf"] = int((f == np.inf).all(axis=0).sum())
    if op in ("max", "min"):
        raw = np.stack([np.ascontiguousarray(s).view(np.uint8).reshape(n, -1) for s in srcs])
        tie = (raw == raw[0]).all(axis=(0, 2))
        out["fourth_elements_tied"] = bool(tie[np.arange(n) % 4 == 1].all())
    if t in O.INT_TYPES:
        ii = np.iinfo(dtype(t))
        allv = np.stack(srcs)
        out["has_min"] = bool((allv == ii.min).any())
        out["has_max"] = bool((allv == ii.max).any())
        if op == "prod":
            exact = np.ones(n, object)
            for s in srcs:
                exact = exact * np.asarray(s).astype(object)
            out["wraps"] = int(sum(1 for x in exact if not ii.min <= x <= ii.max))
            out["small"] = int(sum(1 for x in exact if ii.min <= x <= ii.max and x != 0))
    if t == "longdouble":
        rows = {bytes(r) for r in O.special_values("longdouble").view(np.uint8).reshape(-1, 16)[-4:, :10]}
        seen = {bytes(r) for s in srcs for r in np.ascontiguousarray(s).view(np.uint8).reshape(-1, 16)[:, :10]}
        out["x87_only_rows"] = len(rows & seen)
    return out


# ------------------------------------------------- the collective: one driver
NPES, START, LOG, SIZE = 4, 1, 0, 3          # members 1, 2, 3 of a 4-PE team: PE 0 stays out
HEAP = 1 << 20

_TEAMS = {}


def team(device: bool, host_fold: bool = False, npes: int = NPES):
    """The cached Team of a heap kind (and PE count), made the active one."""
    from support import team as T
    key = (device, npes)
    if key not in _TEAMS:
        _TEAMS[key] = T.Team(npes, HEAP, device=device)
    tm = _TEAMS[key]
    tm.host_fold = host_fold
    tm.activate()
    return tm


def _align(x, a=256):
    return (x + a - 1) // a * a


class DoorCase:
    """One collective call of `door` for (t, op) on the set (start, log, size)
    of an npes-PE team: what to write into every PE's heap (writes[pe]: (offset,
    array)), the call's offsets, and what every member must hold afterwards
    (wants[pe]: (offset, array, type name)).  Sources and targets sit `shift`
    elements off a 256-byte boundary.  null: the location door without index
    sources."""

    def __init__(self, door, t, op, n, seed, npes=NPES, start=START, log=LOG, size=SIZE, shift=1,
                 null=False, lens=None):
        self.door, self.t, self.op, self.n, self.null = door, t, op, n, null
        self.npes, self.set = npes, (start, log, size)
        self.members = O.active_set(start, log, size)
        s = esize(t)

        def spread(member_arrays, other_seed, length, indices=False):
            """Per-PE arrays: the members' in set order; a non-member holds
            inputs of its own, which no result may show."""
            arrs = [None] * npes
            for m, pe in enumerate(self.members):
                arrs[pe] = member_arrays[m]
            for pe in range(npes):
                if arrs[pe] is None:
                    arrs[pe] = np.full(length, 1000 + pe, np.int32) if indices else \
                        matrix_inputs(t, op, 2, length, other_seed + pe)[0]
            return arrs

        self.writes = {pe: [] for pe in range(npes)}
        self.wants = {pe: [] for pe in self.members}
        if door == "many":
            self.lens = list(lens)
            both = {i: shift for i, ln in enumerate(self.lens) if ln > 0}
            self.lay = M.Layout(t, self.lens, odd=both, sodd=both)
            self.bytes = self.lay.bytes
            for i, ln in enumerate(self.lens):
                src = spread(matrix_inputs(t, op, size, ln, seed + 7 * i), seed + 99 + i, ln)
                if ln == 0:
                    continue
                want = C.to_all(t, op, src, start, log, size)
                for pe in range(npes):
                    self.writes[pe].append((self.lay.soff[i], src[pe]))
                for pe in self.members:
                    self.wants[pe].append((self.lay.toff[i], want[pe], t))
            return
        if door == "loc":
            vals = spread(L.tie_values(t, size, n, seed), seed + 99, n)
            locs = spread(L.tie_indices(size, n, seed), 0, n, indices=True) if not null else None
            area = _align(n * max(s, 4) + 16) + 256
            self.soff, self.lsoff = 256 + shift * s, 256 + area + shift * 4
            self.toff, self.ltoff = 256 + 2 * area + shift * s, 256 + 3 * area + shift * 4
            self.bytes = 256 + 4 * area + 4096
            idx = L.const_indices(self.members, n) if null else [locs[pe] for pe in self.members]
            wv, wi = L.expected(t, op, [vals[pe] for pe in self.members], idx)
            for pe in range(npes):
                self.writes[pe].append((self.soff, vals[pe]))
                if not null:
                    self.writes[pe].append((self.lsoff, locs[pe]))
            for pe in self.members:
                self.wants[pe] += [(self.toff, wv, t), (self.ltoff, wi, "int")]
            return
        nsrc = n * size if door == "rscatter" else n
        src = spread(matrix_inputs(t, op, size, nsrc, seed), seed + 99, nsrc)
        self.soff = 256 + shift * s
        self.toff = self.soff + _align(nsrc * s + 16) + 256
        self.bytes = self.toff + _align(n * s + 16) + 4096
        if door == "rscatter":
            want = C.expected(t, op, src, n, start, log, size)
        elif door in ("scan_inc", "scan_exc"):
            want = S.expected(t, op, src, door == "scan_exc", start, log, size)
        elif door == "uniform":
            want = U.expected(t, op, src, start, log, size)
        else:
            raise ValueError(door)
        for pe in range(npes):
            self.writes[pe].append((self.soff, src[pe]))
        for pe in self.members:
            self.wants[pe].append((self.toff, want[pe], t))

    def team_path(self) -> str:
        """What osgpu_last_path() names on device heaps under OSGPU_PATH_AUTO,
        as the per-door tests expect it: the reduce-scatter and the batched
        call have no team kernel; the scan has none for long double."""
        if self.door in ("rscatter", "many"):
            return "pull"
        if self.door in ("scan_inc", "scan_exc") and self.t == "longdouble":
            return "pull"
        return "team"

    def target_mask(self) -> np.ndarray:
        m = np.zeros(self.bytes, bool)
        for off, arr, tt in self.wants[self.members[0]]:
            m[off:off + len(arr) * esize(tt)] = True
        return m


def run_door(tm, case: DoorCase):
    """The call of `case` on team `tm`, every member on its own thread, through
    the case module's run; Team._on_members checks pSync afterwards."""
    start, log, size = case.set
    t, op, n = case.t, case.op, case.n
    if case.door == "rscatter":
        return C.run(tm, t, op, case.toff, case.soff, n, start, log, size)
    if case.door in ("scan_inc", "scan_exc"):
        return S.run(tm, t, op, case.door == "scan_exc", case.toff, case.soff, n, start, log, size)
    if case.door == "uniform":
        return U.run(tm, t, op, case.toff, case.soff, n, start, log, size)
    if case.door == "many":
        return M.run_many(tm, t, op, case.lay, start, log, size)
    if case.door == "loc":
        return L.run(tm, t, op, case.toff, case.ltoff, case.soff, None if case.null else case.lsoff,
                     n, start, log, size)
    raise ValueError(case.door)
