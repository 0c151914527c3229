"""A-priori, per-element error bounds for one step under precision "medium"   --  TEST INFRASTRUCTURE ONLY.

Not an emulation of the kernels' pieces: a first-order perturbation bound, evaluated in numpy float64 on the float64 oracle's own
quantities.  For one head, with the batch X [b, M], the head's P [M, K] and the Q [b, K] the engine actually used:

    R = Q.P^T     dR = (R - X) / (R (1 - R))     S = |d dR / d R|     A = |dR|^T.|Q|

    B_dP = 1.25 . [ (u8 |dR| + 2 u16 R S)^T.|Q|  +  u16 A  +  b 2^-24 A ]                       [M, K]
    B_Z  = 1.25 . u16 . |X|.|V| + 1e-5                                                        [b, C]

u8 = 2^-8: dR enters dP as ONE bf16 piece, rounded to nearest even (8 significant bits: unit roundoff 2^-8).
u16 = 2^-15: P, Q and V enter as two bf16 pieces, hi + mid, the lo piece of the three-way split dropped.  As read from the code:
    * P and Q (pass 2 and the Q images): csrc/nadm_common.h, split3, and its twin split3_pair -- every piece is a round-to-nearest-even
      conversion (pk_bf16, v_cvt_pk_bf16_f32) of what the pieces before it left: |v - hi| <= 2^-8 |v|, |v - hi - mid| <= 2^-16 |v|.
    * V (pass 1, encode_fwd_mfma_kernel): pieces cut by bit truncation (bf16_trunc_bits): v - hi < 2^-7 |v| lies at least eight
      binades below v, and its own cut leaves less than 2^-7 of that binade: |v - hi - mid| < 2^-15 |v|.
    So u16 is exactly the truncating split's bound and twice the rounding split's.  R = Q.P^T is then off by at most 2 u16 R to first
    order (P >= 0, Q >= 0: |Q|.|P|^T = R), which dR sees through S; Q as dR's partner in dP is off by u16 |Q|: the u16 A term.
b 2^-24: the fp32 accumulation over the b samples.   1.25: the second-order terms.
1e-5 in B_Z: the absolute tolerance the "highest" suite asserts on Z (test_step_against_oracle_random_shapes).

Valid where neither the clamp of R to [0, 1] nor the 1e-12 floor of R (1 - R) is active: callers keep P in [0.02, 0.98] and take Q from
the softmax, so R lies in [0.02, 0.98].  Missing calls are x = 0 like everywhere else.

``restate_dp`` / ``restate_z`` are the numpy restatement of the roundings the bound is about (hi + mid operands, fp32 products, dR
rounded to bf16, fp32 accumulation in sample order); the CPU tests of tests/test_precision_medium_shapes.py hold the bound against them
and against planted defects, the GPU tests hold the kernels to the bound.
"""
import numpy as np

U8 = 2.0 ** -8
U16 = 2.0 ** -15
ACC = 2.0 ** -24
SECOND_ORDER = 1.25
Z_ABS = 1e-5
TILE = 64                     # samples per tile of pass 2 (NADM_BF_TS)

# (b, M, ks): the shapes of the medium suite and what each one is there for
SHAPES = [
    (1, 5, [2]),                                   # single sample, M < 8
    (23, 1027, [16]),                              # ragged single tile, M % 4 = 3, both k slots full
    (65, 2049, [5]),                               # one row past a tile, one SNP past a chunk
    (150, 2301, [3]),                              # one-MFMA form, three tiles, the last of 22 rows
    (150, 2301, [8]),                              # K <= 8 form over the same three tiles
    (150, 2301, [13]),                             # two k slots, three pad columns
    (130, 1531, [9]),                              # KP = 12
    (70, 2600, [2, 3, 4, 5, 6, 7, 8, 9, 10]),      # multi-head
    (520, 2301, [4, 8, 12]),                       # nine tiles, the last of 8 rows; pass 2 in slices by the library's own rule
    (900, 1300, [4]),                              # two row blocks in pass 1, sliced pass 2
    (37, 1900, [4]),                               # 60 % missing, one all-missing sample, eight all-missing SNP columns
]
MISSING_HEAVY = (37, 1900, [4])


def shape_id(s):
    return f"{s[0]}x{s[1]}-k{'_'.join(str(k) for k in s[2])}"


# ------------------------------------------------------------------------------------------------ float64 quantities and the bounds
def decode_x64(G):
    X = np.asarray(G).astype(np.float64) / 2.0
    X[np.asarray(G) == 3] = 0.0
    return X


def head64(X, P, Q):
    """float64 (R, dR, dP) of one head: P [M, K], Q [b, K], X [b, M]."""
    X, P, Q = (np.asarray(a, dtype=np.float64) for a in (X, P, Q))
    R = Q @ P.T
    dR = (R - X) / (R * (1.0 - R))
    return R, dR, dR.T @ Q


def dp_bound(X, P, Q, u8=U8, u16=U16):
    """B_dP [M, K] and the float64 dP it is a bound about."""
    X = np.asarray(X, dtype=np.float64)
    R, dR, dP = head64(X, P, Q)
    assert R.min() > 0.0 and R.max() < 1.0, "the bound holds only where no clamp or floor is active"
    den = R * (1.0 - R)
    S = np.abs((den - (R - X) * (1.0 - 2.0 * R)) / (den * den))          # |d/dR (R - X) / (R - R^2)|
    aQ = np.abs(np.asarray(Q, dtype=np.float64))
    A = np.abs(dR).T @ aQ
    b = X.shape[0]
    return SECOND_ORDER * ((u8 * np.abs(dR) + 2.0 * u16 * R * S).T @ aQ + u16 * A + b * ACC * A), dP


def z_bound(X, V, u16=U16):
    """B_Z [b, C] and the float64 Z = X.V."""
    X, V = np.asarray(X, dtype=np.float64), np.asarray(V, dtype=np.float64)
    return SECOND_ORDER * u16 * (np.abs(X) @ np.abs(V)) + Z_ABS, X @ V


def worst(err, B):
    """(max err / B, its index) -- a zero bound with a zero error counts as 0, with a non-zero error as inf."""
    err, B = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(B, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / B)
    r = np.where(np.isfinite(r) | (r == np.inf), r, np.inf)               # NaN (a non-finite entry) is a violation
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(x) for x in i)


def check_dp(got_padded, K, dP64, B):
    """The check the GPU tests apply to one head's dP as the engine holds it, [M, KP] with KP - K pad columns: finite, pad columns exactly
    zero, every entry within B of the float64 dP.  Returns (ok, worst ratio, (SNP, k) of the worst entry, flagged share of the entries)."""
    got = np.asarray(got_padded, dtype=np.float64)
    if not np.isfinite(got).all() or got[:, K:].any():
        return False, float("inf"), (-1, -1), 1.0
    err = np.abs(got[:, :K] - dP64)
    ratio, at = worst(err, B)
    return ratio <= 1.0, ratio, at, float((err > B).mean())


# ------------------------------------------------------------------------------------------------ the roundings, restated
def bf16_rne(x):
    """float32 -> the nearest bf16 value (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_trunc(x):
    """float32 -> the bf16 value below it in magnitude (the upper 16 bits), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def hi_mid(x, cut=bf16_rne):
    """The first two pieces of a three-way split added up (exact in fp32: at most 16 significant bits).  ``cut`` makes a piece:
    bf16_rne is split3 (csrc/nadm_common.h: P and Q), bf16_trunc pass 1's split of V."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = cut(x)
    return h + cut(x - h)


def restate_dp(X, P, Q, cut=bf16_rne):
    """dP [M, K] in fp32 with the medium step's roundings: P and Q as hi + mid, R = Q.P^T as an fp32 product, dR in fp32 and then ONE
    bf16 piece (nearest even), dP accumulated in fp32 one sample after the other (the longest chain an fp32 sum over the batch can
    have).  ``cut`` = bf16_trunc restates the operands at the full u16 the bound grants them instead of split3's 2^-16."""
    Pt, Qt = hi_mid(P, cut), hi_mid(Q, cut)
    X32 = np.asarray(X, dtype=np.float32)
    R = (Qt @ Pt.T).astype(np.float32)
    dR = bf16_rne(((R - X32) / (R * (np.float32(1) - R))).astype(np.float32))
    acc = np.zeros((Pt.shape[0], Qt.shape[1]), dtype=np.float32)
    for i in range(X32.shape[0]):
        acc += np.outer(dR[i], Qt[i])
    return acc


def restate_z(X, V):
    """Z [b, C] in fp32 with V as the hi + mid of pass 1's truncating split (X is exact in bf16)."""
    return (np.asarray(X, dtype=np.float32) @ hi_mid(V, bf16_trunc)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ planted defects
def planted_defects(X, P, Q, KP):
    """Defects a pass 2 could have at this shape, planted in the float64 oracle's dP: name -> [M, KP] array (pad columns zero unless the
    defect is about them).  Every one must be rejected by ``check_dp``."""
    _, dR, dP = head64(X, P, Q)
    Q = np.asarray(Q, dtype=np.float64)
    b, K = Q.shape
    M = dP.shape[0]

    def padded(a):
        out = np.zeros((M, KP))
        out[:, :K] = a
        return out

    out = {}
    if b % TILE:
        out["last_sample_of_ragged_tile_dropped"] = padded(dP - np.outer(dR[b - 1], Q[b - 1]))
    d = dP.copy()
    d[M - 1] = 0.0
    out["last_snp_dropped"] = padded(d)
    t = min(b, TILE)
    out["first_tile_twice"] = padded(dP + dR[:t].T @ Q[:t])
    if K - 1 > 8:                                       # (K = 9: columns 8 and K - 1 are the same column, nothing to plant)
        d = dP.copy()
        d[:, [8, K - 1]] = d[:, [K - 1, 8]]
        out["columns_8_and_last_swapped"] = padded(d)
    if KP > K:
        d = padded(dP)
        d[M // 2, K] = 1e-30
        out["pad_column_nonzero"] = d
    return out


def required_defects(b):
    """Which planted defects a shape must catch.  One sample among b >= 900 moves dP by less than dR's one bf16 piece allows the whole sum
    to be off, entry by entry: there the duplicated tile and the dropped SNP are required, below (b <= 520) every defect that applies."""
    if b >= 900:
        return {"last_snp_dropped", "first_tile_twice"}
    return {"last_sample_of_ragged_tile_dropped", "last_snp_dropped", "first_tile_twice", "columns_8_and_last_swapped", "pad_column_nonzero"}


# ------------------------------------------------------------------------------------------------ the cases' inputs
def make_case(O, b, M, ks, Hd=64, C=8):
    """Inputs of one case, the same for the CPU and the GPU tests: genotypes of b + 40 samples (5 % missing), a permutation of the rows
    whose first b are the batch, V ~ N(0, 1/M), P uniform in [0.02, 0.98].  ``O`` is the oracle module."""
    seed = 1000 + 7 * b + M + sum(ks)
    heavy = (b, M, list(ks)) == (MISSING_HEAVY[0], MISSING_HEAVY[1], MISSING_HEAVY[2])
    Gm = O.synth_genotypes(b + 40, M, max(2, min(max(ks), 6)), seed=seed, missing=0.6 if heavy else 0.05)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(b + 40).astype(np.int32)
    if heavy:                                           # the missing-heavy case of the "highest" suite
        Gm[perm[5], :] = 3                              # batch row 5: not a single call
        Gm[:, 100:108] = 3
    V0 = (rng.standard_normal((M, C)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.02, 0.98, size=(sum(ks), M)).astype(np.float32)
    p = O.make_params(seed % 97, V0, P0, Hd, ks)
    return Gm, perm, p
