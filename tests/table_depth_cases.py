"""MSM base sets with a table depth (h2mi_bases_register_depth, csrc/h2mi_msm.hip "table depth"), shared by
tests/test_table_depth_host.py and tests/test_gpu_table_depth.py: a Python model of the signed recoding (for_each_digit), of the pass
and table row every window is given at depth D, and of the bytes register_dev asks the allocator for; the edge scalars
for a window width; and the scalar columns of the device tests.  Bases and expected results are those of tests/msm_schedule_cases.py
(random multiples of the generator, sums by oracle/cref.py).  With H2MI_MSM_C in the environment (the wide-window runs, in a child
process) the model takes that width, as the library does for every registration of the process."""
import functools
import os

import numpy as np

import msm_schedule_cases as S
from oracle import bn254 as o

R = o.R
FORCED_C = int(os.environ.get("H2MI_MSM_C", "0"))

# ---- the constants of csrc/h2mi_msm.hip and csrc/scan.cuh, restated -------------------------------------------------------------------
PART_BYTES = 144  # one XYZZ partial sum
P1_TS = 768  # scalars per partition tile
S1 = 8  # partials per fold task
ACCUM_RESIDENT_CHUNKS = 256 * 2 * 256
S0_MAX = 128
MAT_LOG = 16  # the bucket matrix holds 2^16 buckets; wider windows add a segment level
SCAN_SEG_BINS = 8192
SHIFT_MIN_N = 4096
SIZES = (1, 2, 767, 769, 4095, 4096, 4097, (1 << 13) + 1)


def window(n: int) -> int:
    """window bits of a base set of n points"""
    return FORCED_C or S.pick_window(n)


def windows(c: int) -> int:
    return -(-255 // c)


def depths(W: int) -> list:
    """the table depths the tests register: 1, the small ones, both sides of W and one beyond"""
    return sorted({1, 2, 3, 4, W - 1, W, W + 5})


# ---- the recoding and the pass scheme ---------------------------------------------------------------------------------------------------
def recode(s: int, c: int) -> list:
    """for_each_digit: the W signed digits of the canonical scalar s, d_w in (-2^(c-1), 2^(c-1)], s = sum_w d_w 2^(c w)"""
    assert 0 <= s < R
    W, half, out, carry = windows(c), 1 << (c - 1), [], 0
    for w in range(W):
        d = ((s >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 0
        if d > half:
            d -= 1 << c
            carry = 1
        out.append(d)
    assert carry == 0
    return out


def effective(D: int, W: int) -> tuple:
    """(D', rows) of a registration at depth D"""
    Dp = min(D, W)
    return Dp, -(-W // Dp)


def pass_of(w: int, Dp: int) -> int:
    return w % Dp


def row_of(w: int, Dp: int) -> int:
    return w // Dp


def pass_digits(s: int, c: int, D: int) -> list:
    """per pass r < D': the (table row, digit) pairs the pass inserts for the scalar s — its own windows' non-zero digits"""
    Dp, _ = effective(D, windows(c))
    out = [[] for _ in range(Dp)]
    for w, d in enumerate(recode(s, c)):
        if d:
            out[pass_of(w, Dp)].append((row_of(w, Dp), d))
    return out


def recombine(s: int, c: int, D: int) -> int:
    """sum_r 2^(c r) sum_(w = r mod D') d_w 2^(c D' floor(w / D')): what the passes and k_msm_combine compute, as an integer"""
    Dp, _ = effective(D, windows(c))
    return sum((1 << (c * r)) * sum(d << (c * Dp * row) for row, d in entries) for r, entries in enumerate(pass_digits(s, c, D)))


def insertions(scalars, c: int) -> int:
    """bucket insertions of an MSM without a shift: the non-zero digits of its scalars"""
    return sum(1 for s in scalars for d in recode(s, c) if d)


# ---- the edge scalars -------------------------------------------------------------------------------------------------------------------
def edge_scalars(c: int) -> dict:
    """name -> scalar, for window width c: the ends of the field, and for every window w the all-ones value below it 2^(c w) - 1 (a
    carry through every window up to w), 2^(c w + c - 1) (the digit that is exactly 2^(c-1), the largest positive one), that plus 1,
    and (2^(c-1) + 1) 2^(c w) (the first negative digit in window w, a carry into the next)"""
    W = windows(c)
    out = {"0": 0, "1": 1, "r-1": R - 1, "(r-1)/2": (R - 1) // 2}
    for w in range(W):
        for name, v in ((f"2^(c{w})-1", (1 << (c * w)) - 1), (f"half at {w}", 1 << (c * w + c - 1)), (f"half at {w}, plus 1", (1 << (c * w + c - 1)) + 1),
                        (f"half+1 at {w}", ((1 << (c - 1)) + 1) << (c * w))):
            if 0 <= v < R:
                out[name] = v
    return out


def one_class_scalars(c: int, D: int, q: int) -> list:
    """scalars whose non-zero digits all lie in the windows w = q mod D': every other pass has no entry for them.  Positive and
    negative digits, the extremes included, the top one positive (the scalar is then positive and its recoding is these digits)"""
    W = windows(c)
    Dp, _ = effective(D, W)
    half = 1 << (c - 1)
    ws = [w for w in range(q % Dp, W) if w % Dp == q % Dp and c * w <= 250]
    assert ws
    pattern = [half, -(half - 1), 1, -1, 3 - half, half - 2]
    out = []
    for start in range(3):
        digits = {w: pattern[(start + i) % len(pattern)] if c * w + c <= 252 else 1 for i, w in enumerate(ws)}  # (stay below r)
        digits[ws[-1]] = abs(digits[ws[-1]])
        out.append(sum(d << (c * w) for w, d in digits.items()))
        out.append(abs(digits[ws[0]]) << (c * ws[0]))  # a single digit
    assert all(0 < s < R for s in out)
    return out


# ---- the bytes a handle holds -----------------------------------------------------------------------------------------------
def _accum_rounds(entries: int) -> int:
    per_round = S0_MAX * ACCUM_RESIDENT_CHUNKS
    return -(-entries // per_round) if entries else 1


def memory(n: int, D: int) -> tuple:
    """(D', rows, table bytes, workspace bytes) of a base set of n points registered at depth D, as register_dev asks for them:
      table     = rows (n + 1) 64                                   [+ the latency path's 2^(cs-1) Ws n 64 at depth 1, n <= 2^14]
      workspace = slots x (entries x (8 + key bytes) + bins + bucket tables + partial sums + reduction scratch) [+ W 96 at depth > 1]
    with entries = rows (n + 1) and one slot at depth > 1, W (n + 1) and eight (four above 2^17 points) at depth 1"""
    c = window(n)
    W = windows(c)
    Dp, rows = effective(D, W)
    stride = n + 1
    nW = stride * rows
    nb = 1 << (c - 1)
    seg_log = max(c - 1 - MAT_LOG, 0)
    logNl = (c - 1 - seg_log + 1) // 2
    logNh = (c - 1 - seg_log) - logNl
    lb = max(c - 1 - 9, 0)
    nbins = nb >> lb
    max_tasks0 = min(_accum_rounds(nW) * ACCUM_RESIDENT_CHUNKS, nW) + nb + 1
    max_tasks1 = max_tasks0 // S1 + nb
    ntiles = -(-stride // P1_TS)
    bin_cells = nbins * ntiles + 1
    slot = 2 * nW * 4 + nW * (2 if seg_log else 1) + 16  # payloads by bin and by bucket, in-bin keys
    slot += 2 * bin_cells * 4 + (bin_cells // SCAN_SEG_BINS + 2) * 4 + (ntiles + 1) * 4  # [bin][tile] counts, their scan, segment sums, live tiles
    slot += (nb + 1) * 4 + 4 + 4 * (nb + 1) * 4  # bucket offsets, chunk length, task counts and their scans
    slot += nb * PART_BYTES  # one sum per bucket
    if seg_log:
        slot += 2 * (1 << MAT_LOG) * PART_BYTES + 2 * (nb // SCAN_SEG_BINS + 2) * 4
    slot += (max_tasks0 + max_tasks1) * PART_BYTES  # partial sums of the accumulation and of the fold
    slot += ((2 << logNh) + (1 << logNl)) * PART_BYTES + 64 * PART_BYTES  # row / column sums, weighted partials
    slot += (256 if Dp > 1 else 64) + 32  # statistics, the shift value
    nslot = 1 if Dp > 1 else 4 if n > (1 << 17) else S.NSLOT
    table = nW * 64
    work = nslot * slot + (W * 96 if Dp > 1 else 0)  # the pass results
    g = S.small_geometry(n)
    if Dp == 1 and g.table and not FORCED_C:  # the latency path's table and digit / partial-sum scratch
        table += g.table_bytes
        work += nslot * (g.W * n + g.G * PART_BYTES + (g.G + 1) * 4)
    return Dp, rows, table, work


# ---- the scalar columns of the device tests -----------------------------------------------------------------------------------------------
FIXED_COLUMNS = ("edges", "shift3", "bits", "uniform")


def _cycle(values: list, n: int) -> np.ndarray:
    return o.pack([values[i % len(values)] for i in range(n)], R)


@functools.lru_cache(maxsize=None)
def column(n: int, name: str, D: int = 0) -> np.ndarray:
    """(n, 4) Montgomery limbs, read-only.  "edges": the edge scalars of the size's window width, in turn; "one_class" (depends on D):
    only scalars whose digits lie in the windows 1 mod D', so that every other pass of the MSM is empty; "shift3": one value on all but
    three rows; "bits": zeros and ones; "uniform"."""
    c = window(n)
    if name == "edges":
        a = _cycle(list(edge_scalars(c).values()), n)
    elif name == "one_class":
        a = _cycle(one_class_scalars(c, D, 1), n)
    elif name == "shift3":
        a = S.column(n, "repeated3")
    elif name == "bits":
        a = o.pack([int(b) for b in np.random.default_rng(4400 + n).integers(0, 2, n)], R)
    elif name == "uniform":
        a = S.column(n, "uniform")
    else:
        raise KeyError(name)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def columns(D: int) -> list:
    """the (name, D-key) pairs of every case column at depth D"""
    return [(name, 0) for name in FIXED_COLUMNS] + [("one_class", D)]


@functools.lru_cache(maxsize=None)
def expected(n: int, name: str, D: int, length: int) -> bytes:
    """affine limbs of sum_(i < length) column[i] * bases[i], from the C restatement: once per (column, length)"""
    from oracle import cref

    return cref.normalize(cref.msm(column(n, name, D)[:length], S.bases()[:length], 4)).tobytes()
