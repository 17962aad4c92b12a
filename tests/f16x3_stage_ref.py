"""
CPU reference of compute mode f16x3's split kernels (not a test, not a conftest: a helper of tests/test_f16x3_stage_ref.py and
tests/test_gpu_f16x3_stages.py).  It restates, bit for bit, what the split passes write (scfgp_amd/csrc/gram_f16.hip:
split_rows_kernel; apply_f16.hip: split_operand_kernel and the plane stores of V = Phi B's epilogue), forms the three-term products
exactly in fp64 from the planes, and reports normalised errors per block of the output.

Plane form (kernels.h): 4 bytes per element; per 16 consecutive columns the 16 fp16 h's, then the 16 l's.

The rules restated here:
  rows (split_rows_kernel)      e = 14 - ilogb(bound) (bound an fp32 number), xs = x 2^e in fp32, h = fp16(xs), l = fp16(xs - h)
  rows times q[n] (qV16g)       e1 = 14 - ilogb(fp32(bound_V * maxq)), f = fp32(q[n] 2^e1), xf = fp32(x f), h = fp16(xf),
                                l = fp16(xf - h)
  operand (split_operand_kernel) em = 14 - ilogb(max |M|) in fp64, x = M^T 2^em in fp64, h = fp16(x), l = fp16(x - h) (single
                                roundings from fp64), scale[0] = 2^-(em + e_Phi), e_Phi = 14 - ilogb(fp32(s)), scale[1] = 2^em
  Gram product                  slab = scale (Ah^T Bh + Al^T Bh + Ah^T Bl) on the lower 128-tiles; the upper tiles are the mirror
  apply product                 V = scale (Phih Bh^T + Phil Bh^T + Phih Bl^T), B16's row j = output column j
"""
import numpy as np

F16_TILE = 128              # square tiles of the Gram products and of the exchange layout
APPLY_BM = 256              # rows per block of the apply tiles and of the split passes' granule
FOLD = 512                  # rows after which the fp16 Gram's fp32 chains are folded into the second accumulator set


# ---- tolerances of the GPU stage walk (tests/test_gpu_f16x3_stages.py); tests/test_f16x3_stage_ref.py shows that each one
# passes a correct emulated result and fails every mutation visible at its stage by at least 10x --------------------------------
# normalised error (|X - X3| / (|A|^T |B|) element-wise, worst block) of a product against its exact three-term value from the
# planes: accumulation error only.  Worst figures of the walk on an MI355X: G 5.9e-7 (K = 132, 257 rows: one 256-row fold), W 3.5e-7,
# V 7.2e-7 and 2 Phi Abar 3.9e-7 (K = 4224); every mutation of tests/test_f16x3_stage_ref.py lands at 2e-5 or above
CAP_GRAM3 = 2e-6
CAP_APPLY3 = 2e-6
# the 4x rule against the exact product of the fp32 operands: err16 <= 4 err32 + FLOOR_SPLIT (the split's own floor: h + l
# represents an fp32 value to 2^-22 of itself and the dropped l.l term is 2^-22 of |a||b|)
FLOOR_SPLIT = 2.0 ** -20
RULE = 4.0
OUTLIER = 8.0               # no block's figure above 8x the median of blocks of its kind (plus the cap's 1 %)


def ilogb(x):
    """C's ilogb for finite x != 0 (float32 or float64 alike: the exponent does not depend on the precision here)."""
    return int(np.frexp(float(x))[1]) - 1


def exponent(bound):
    """e = 14 - ilogb(bound) (0 for bound <= 0): the scale that puts |x| <= bound into [.., 2^15)"""
    b = float(np.float32(bound))
    return 14 - ilogb(b) if b > 0 else 0


# ---- plane form ------------------------------------------------------------------------------------------------------------
def decode_planes(words):
    """(R x Kp) uint32 (or R x 4 Kp bytes) in plane form -> (h, l) as float16 arrays of R x Kp"""
    w = np.ascontiguousarray(words)
    R = w.shape[0]
    a = w.view(np.float16).reshape(R, -1)
    Kp = a.shape[1] // 2
    a = a.reshape(R, Kp // 16, 2, 16)
    return a[:, :, 0, :].reshape(R, Kp).copy(), a[:, :, 1, :].reshape(R, Kp).copy()


def encode_planes(h, l):
    R, Kp = h.shape
    a = np.empty((R, Kp // 16, 2, 16), np.float16)
    a[:, :, 0, :] = h.reshape(R, Kp // 16, 16); a[:, :, 1, :] = l.reshape(R, Kp // 16, 16)
    return a.reshape(R, 2 * Kp).view(np.uint32)


def planes_value(h, l, e):
    """(h + l) 2^-e in fp64 (exact)"""
    return (h.astype(np.float64) + l.astype(np.float64)) * 2.0 ** -e


# ---- the device's split rules ------------------------------------------------------------------------------------------------
def split_rows(M32, bound):
    """split_rows_kernel's plain output: h, l, e"""
    e = exponent(bound)
    xs = np.asarray(M32, np.float32) * np.float32(2.0 ** e)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)
    return h, l, e


def split_rows_weighted(M32, q, bound, maxq, model='plain'):
    """split_rows_kernel's weighted output (diag(q) M, qV16g): h, l, e1.  bound = f16tmp[5], maxq = f16tmp[6].
      plain  what the kernel does: xf = fp32(x f), h = fp16(xf), l = fp16(xf - h)
      mix    what it did while the compiler folded the product into v_fma_mix*_f16: l = fp16(x f - h') rounded once from the exact
             x f - h', h' = fp16(x f) rounded once from the exact product -- not the h it stores (kept to show the difference)"""
    b1 = np.float32(bound) * np.float32(maxq)
    e1 = exponent(b1)
    f = (np.asarray(q, np.float64) * 2.0 ** e1).astype(np.float32)
    M32 = np.asarray(M32, np.float32)
    y = M32 * f[:, None]
    h = y.astype(np.float16)
    if model == 'mix':
        xf = M32.astype(np.float64) * f.astype(np.float64)[:, None]
        l = (xf - xf.astype(np.float16).astype(np.float64)).astype(np.float16)
    else:
        l = (y - h.astype(np.float32)).astype(np.float16)
    return h, l, e1


def split_operand(M, K, s):
    """split_operand_kernel: (h, l) of Kp x Kp (row j = column j of M, zero beyond K), scale[0], scale[1]"""
    M = np.asarray(M, np.float64)
    Kp = M.shape[0]
    m = np.abs(M[:K, :K]).max()
    em = 14 - ilogb(m) if m > 0 else 0
    ephi = 14 - ilogb(np.float32(s))
    x = np.zeros((Kp, Kp))
    x[:K, :K] = np.ldexp(M[:K, :K].T, em)
    h = x.astype(np.float16)
    l = (x - h.astype(np.float64)).astype(np.float16)
    return h, l, 2.0 ** -(em + ephi), 2.0 ** em


def v_bound(B, K, s, M):
    """v_bound_kernel: s sqrt(M) max_j |B_j| (1 + 1e-6) as an fp32 number (its fp64 row sums may differ from these in the last bits)"""
    return float(np.float32(s * np.sqrt(M) * np.sqrt((np.asarray(B)[:K, :K] ** 2).sum(1)).max() * (1.0 + 1e-6)))


# ---- exact three-term products -----------------------------------------------------------------------------------------------
def _f(x):
    return x.astype(np.float64)


def gram3(Ah, Al, Bh, Bl, scale):
    """scale (Ah^T Bh + Al^T Bh + Ah^T Bl) in fp64 (products of fp16 values are exact; the fp64 sums all but so)"""
    return (_f(Ah).T @ (_f(Bh) + _f(Bl)) + _f(Al).T @ _f(Bh)) * scale


def apply3(Ph, Pl, Bh, Bl, scale):
    """scale (Ph Bh^T + Pl Bh^T + Ph Bl^T): V = Phi B with B16's row j = output column j"""
    return (_f(Ph) @ (_f(Bh) + _f(Bl)).T + _f(Pl) @ _f(Bh).T) * scale


def mirror_lower_tiles(P, tile=F16_TILE):
    """the unpacked exchange matrix built from P's lower tiles: tile (i, j) with i >= j as P has it, the upper ones mirrored"""
    n = P.shape[0]
    ti = np.arange(n) // tile
    low = ti[:, None] >= ti[None, :]
    return np.where(low, P, P.T)


# ---- launch geometry, restated from the host code ------------------------------------------------------------------------------
def round_up(x, m):
    return -(-x // m) * m


def apply_plan(K):
    """apply.hip ApplyPlan: (count of 128-wide blocks, col0 and count of the 64-wide ones)"""
    c128 = 0 if K <= 256 else K // 128
    col = 128 * c128
    return c128, col, -(-(K - col) // 64)


def f16_apply_runs(K):
    return apply_plan(K)[0] > 0


def f16_apply_tiles(K, Np, ncu):
    """the f16 apply launch (apply.hip apply_launch with dma = 2): dict(n256, tail_rb, nrb, main = [(col0, width)], tail = [...])"""
    c128, col64, c64 = apply_plan(K)
    nrb = Np // APPLY_BM
    n256 = c128 // 2
    tail_rb = 0
    tiles = nrb * n256
    rem = tiles % ncu
    if n256 > 0 and tiles > ncu and rem > 0 and 20 * rem <= 9 * ncu:
        tail_rb = (rem + n256 - 1) // n256
    main = [(256 * i, 256) for i in range(n256)] + [(256 * n256 + 128 * i, 128) for i in range(c128 - 2 * n256)]
    main += [(col64 + 64 * i, 64) for i in range(c64)]
    tail = [(128 * i, 128) for i in range(c128)] + [(col64 + 64 * i, 64) for i in range(c64)]
    return dict(n256=n256, tail_rb=tail_rb, nrb=nrb, main=main, tail=tail)


def gram_tiles(Kp):
    n = Kp // 128
    return sum(min(2 * ti + 2, n) for ti in range(0, (n + 1) // 2))


def f16_chunk(Np, Kp, gram_chunk=4096):
    """api_ctx.h f16_chunk(): rows per job of the fp16 Gram"""
    top = 2 * gram_chunk if gram_chunk > 0 else 8192
    fill = Np * gram_tiles(Kp) // 512 // 512 * 512
    return max(min(top, fill), 1024)


def gram_chunks(Np, chunk):
    """gram_f16.hip: (rows per chunk after rounding, number of chunks, rows of the last)"""
    if chunk <= 0 or chunk > Np:
        chunk = Np
    chunk = round_up(chunk, 256)
    n = -(-Np // chunk)
    return chunk, n, Np - (n - 1) * chunk


# ---- errors per block ---------------------------------------------------------------------------------------------------------
def normalised(X, X0, scale_abs):
    """|X - X0| / scale_abs element-wise (0 where scale_abs is 0 and X == X0; inf where it is 0 and they differ)"""
    d = np.abs(np.asarray(X, np.float64) - X0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = d / scale_abs
    r[(scale_abs == 0) & (d == 0)] = 0.0
    return r


def block_max(err, row_edges, col_edges):
    """worst element of each block: array [row block, col block]"""
    out = np.zeros((len(row_edges) - 1, len(col_edges) - 1))
    for i in range(len(row_edges) - 1):
        for j in range(len(col_edges) - 1):
            b = err[row_edges[i]:row_edges[i + 1], col_edges[j]:col_edges[j + 1]]
            out[i, j] = b.max() if b.size else 0.0
    return out


def tile_errors(err, K, tile=F16_TILE):
    """per 128 x 128 tile of a K x K result: {(ti, tj): worst}, lower tiles only (the upper ones are their mirrors)"""
    e = np.arange(0, K, tile).tolist() + [K]
    bm = block_max(err[:K, :K], e, e)
    return {(i, j): bm[i, j] for i in range(bm.shape[0]) for j in range(i + 1)}


def apply_errors(err, N, K, tiles=None):
    """per (256-row block, column tile) of an N x K result; tiles = [(col0, width)] (default 128-wide) -> {(rb, col0): worst}"""
    if tiles is None:
        tiles = [(c, min(128, K - c)) for c in range(0, K, 128)]
    out = {}
    for rb in range(-(-N // APPLY_BM)):
        r0, r1 = rb * APPLY_BM, min(N, (rb + 1) * APPLY_BM)
        for c0, w in tiles:
            c1 = min(K, c0 + w)
            if c1 > c0:
                out[(rb, c0)] = float(err[r0:r1, c0:c1].max())
    return out


def worst(blocks):
    """(figure, block index) of the worst block"""
    k = max(blocks, key=lambda t: blocks[t])
    return float(blocks[k]), k


def outliers(blocks, cap, factor=OUTLIER):
    """blocks whose figure exceeds factor x the median of all (plus 1 % of the cap, so that exact blocks do not make noise of 0)"""
    v = np.array(list(blocks.values()))
    lim = factor * np.median(v) + 0.01 * cap
    return {k: x for k, x in blocks.items() if x > lim}


# ---- a model of the device's accumulation (CPU tests: a "correct" result to hold the tolerances against) ------------------------
def gram_device_model(Ah, Al, Bh, Bl, scale, chunk, stage=32, fold=FOLD):
    """fp32 accumulators per chain of `fold` rows, each 32-row stage's three terms added in fp32, chains folded in fp32, chunks
    summed in fp64 (gram_f16.hip); round to nearest where the matrix instruction truncates -- a model, not the device"""
    N = Ah.shape[0]
    out = np.zeros((Ah.shape[1], Bh.shape[1]))
    for c0 in range(0, N, chunk):
        tot = np.zeros_like(out, dtype=np.float32)
        for f0 in range(c0, min(N, c0 + chunk), fold):
            acc = np.zeros_like(tot)
            for s0 in range(f0, min(N, c0 + chunk, f0 + fold), stage):
                sl = slice(s0, min(N, s0 + stage))
                for A, B in ((Ah, Bh), (Al, Bh), (Ah, Bl)):
                    acc = (acc + (_f(A[sl]).T @ _f(B[sl])).astype(np.float32)).astype(np.float32)
            tot = (tot + acc).astype(np.float32)
        out += tot.astype(np.float64) * scale
    return out


def apply_device_model(Ph, Pl, Bh, Bl, scale, stage=32):
    """fp32 accumulator over the k stages of 32, the three terms of a stage added in fp32 (apply_f16.hip)"""
    acc = np.zeros((Ph.shape[0], Bh.shape[0]), np.float32)
    for k0 in range(0, Ph.shape[1], stage):
        sl = slice(k0, k0 + stage)
        for A, B in ((Ph, Bh), (Pl, Bh), (Ph, Bl)):
            acc = (acc + (_f(A[:, sl]) @ _f(B[:, sl]).T).astype(np.float32)).astype(np.float32)
    return (acc * np.float32(scale)).astype(np.float64)
