"""numpy restatement of the fp32 actor's noisy forward: the exploration noise
of k_actor_fwd32 / k_actor_fwd16 (csrc/sk_act32.hpp, actor_tile32 /
actor_tile16) as a pure function of (seed, call, global row, unit).

TEST INFRASTRUCTURE ONLY (see oracle/keras_ref.py): no torch, no GPU, nothing
read from outside the repository.

What the kernels draw, restated:

  * Philox4x32 with `rounds` rounds, counter (row_key, unit, call & 0xFFFFFFFF,
    call >> 32), key (seed & 0xFFFFFFFF, seed >> 32); `call` is the device
    counter's value plus one.
  * normals4: the four words of one draw are two Box-Muller pairs,
        u1 = ((w >> 8) + 0.5) 2^-24   formed in fp32, as the kernel forms it:
                                      above 2^23 the + 0.5 rounds to even and
                                      the top bucket is exactly 1.0 (part of
                                      the definition)
        u2 = (w >> 8) 2^-24           revolutions (exact)
        z  = [r0 cos0, r0 sin0, r1 cos1, r1 sin1],  r = sqrt(-2 ln u1)
    everything after u1 / u2 in the evaluation dtype.
  * Layers 1 and 2: ROUNDS_PARAM = 7 rounds (kF32NoiseRounds), row key
    4 (row // 4), row r takes z[r % 4]; unit u for layer 1, 256 + u for
    layer 2.  Layer 3: 10 rounds, row key = the row, unit 384, outputs 0 / 1
    take z[0] / z[1].  Action noise: 10 rounds, row key = the row, unit 385,
    action_sd z[0:2] added after tanh.
  * Each layer y = x W^T + b + sd sqrt(x^2 (W^2)^T + b^2) xi (the
    distribution of w (1 + sd N(0,1)) per weight and bias,
    SkillshotLearner.py:245-281), relu, the same again, then tanh.
    squares = "exact": x^2 and W^2 as they are (the 16-row tile: an fp32 MFMA
    of fp32 squares); "bf16": layers 1 and 2 on bf16(fl32(x x)) and
    bf16(fl32(w w)), round to nearest even, as sk_split.hpp split4 writes them
    (the 32-row tile); layer 3 is exact in both.

dtype = np.float64 is the reference; np.float32 evaluates the same formulas in
fp32, the floor the keyed tests' bars are set from.  With sd = 0 and
action_sd = 0 the forward is keras_ref.actor_forward's arithmetic.

split_forward models the noise-free 32-row tile's GEMMs (sk_split.hpp): three
bf16 pieces per operand and the six piece products it keeps, summed in fp64.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF
H1, H2 = 256, 128
UNIT_L3, UNIT_ACTION = H1 + H2, H1 + H2 + 1
ROUNDS_PARAM, ROUNDS_FULL = 7, 10


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 with `rounds` rounds on uint64 arrays (or ints) holding
    uint32 values; returns the 4 output words, uint64 arrays of the
    counters' broadcast shape."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(U32) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & U32, int(k1) & U32
    m32, s32 = np.uint64(U32), np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # < 2^64: exact
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c


def draw_words(seed, call, row_key, unit, rounds):
    """the 4 words of the draw keyed (row_key, unit, call; seed) as the
    kernels key it: uint64 [..., 4]"""
    seed, call = int(seed), int(call)
    return np.stack(philox4x32(row_key, unit, call & U32, (call >> 32) & U32, seed & U32, (seed >> 32) & U32, rounds),
                    -1)


def uniforms(words):
    """(u1, u2) of a draw's words [..., 4] -> fp32 arrays [..., 2]: word 2q
    gives pair q's u1, word 2q + 1 its u2"""
    w = (np.asarray(words, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)  # < 2^24: exact
    u1 = (w[..., 0::2] + np.float32(0.5)) * np.float32(2.0 ** -24)  # the fp32 add rounds above 2^23
    u2 = w[..., 1::2] * np.float32(2.0 ** -24)
    return u1, u2


def normals4(words, dtype=np.float64):
    """Box-Muller on a draw's words [..., 4] -> z [..., 4] =
    [r0 cos0, r0 sin0, r1 cos1, r1 sin1] in `dtype`"""
    u1, u2 = uniforms(words)
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    ang = dtype(2.0 * np.pi) * u2
    z = np.empty(u1.shape[:-1] + (4,), dtype=dtype)
    z[..., 0::2] = r * np.cos(ang)
    z[..., 1::2] = r * np.sin(ang)
    return z


def group_normals(seed, call, rows, unit0, units, dtype=np.float64):
    """xi [len(rows), units] of a hidden layer: Philox-7 keyed by the first
    row of the aligned 4-row group and unit0 + u, row r taking z[r % 4]"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    u = np.arange(units, dtype=np.uint64).reshape(1, -1) + np.uint64(unit0)
    z = normals4(draw_words(seed, call, rows & ~np.uint64(3), u, ROUNDS_PARAM), dtype)
    pick = np.broadcast_to((rows & np.uint64(3)).astype(np.int64), z.shape[:-1])[..., None]
    return np.take_along_axis(z, pick, -1)[..., 0]


def row_normals(seed, call, rows, unit, dtype=np.float64):
    """z[0:2] [len(rows), 2] of the Philox-10 draw keyed by the row itself
    (layer 3: unit UNIT_L3; action noise: UNIT_ACTION)"""
    rows = np.asarray(rows, dtype=np.uint64)
    return normals4(draw_words(seed, call, rows, unit, ROUNDS_FULL), dtype)[..., :2]


def param_normals(seed, call, rows, dtype=np.float64):
    """(xi1 [R, 256], xi2 [R, 128], xi3 [R, 2]) of the global rows `rows`"""
    return (group_normals(seed, call, rows, 0, H1, dtype), group_normals(seed, call, rows, H1, H2, dtype),
            row_normals(seed, call, rows, UNIT_L3, dtype))


def action_normals(seed, call, rows, dtype=np.float64):
    return row_normals(seed, call, rows, UNIT_ACTION, dtype)


def bf16_round(a):
    """fp32 array -> the nearest bf16 value (ties to even), as fp32"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def _squares(x, how, dtype):
    if how == "exact":
        return x * x
    if how == "bf16":
        x32 = x.astype(np.float32)
        return bf16_round(x32 * x32).astype(dtype)
    raise ValueError("squares must be 'exact' or 'bf16'")


def noisy_layer(x, W, b, sd, xi, squares, dtype):
    """y = x W^T + b + sd sqrt(x^2 (W^2)^T + b^2) xi in `dtype`"""
    m = x @ W.T + b
    if sd == 0:
        return m
    v = _squares(x, squares, dtype) @ _squares(W, squares, dtype).T + b * b
    return m + dtype(sd) * np.sqrt(v) * xi


def forward_with_normals(P, s, sd, xi, action_sd=0.0, za=None, squares="exact", dtype=np.float64, var_scale=1.0):
    """the noisy forward on given normals xi = (xi1, xi2, xi3) and action
    normals za [R, 2]; var_scale multiplies the variance sums (1.0: the
    definition; tests perturb it)"""
    Q = {k: np.asarray(v).astype(dtype) for k, v in P.items()}
    x = np.asarray(s).astype(dtype)
    sdv = dtype(sd) * dtype(np.sqrt(var_scale))
    h = np.maximum(noisy_layer(x, Q["l1.weight"], Q["l1.bias"], sdv, xi[0] if sd else None, squares, dtype), 0)
    h = np.maximum(noisy_layer(h, Q["l2.weight"], Q["l2.bias"], sdv, xi[1] if sd else None, squares, dtype), 0)
    a = np.tanh(noisy_layer(h, Q["l3.weight"], Q["l3.bias"], sdv, xi[2] if sd else None, "exact", dtype))
    if action_sd:
        a = a + dtype(action_sd) * za
    return a


def actor_forward_noisy(P, s, sd, action_sd, seed, call, row0=0, squares="exact", dtype=np.float64):
    """actions [R, 2] of rows row0 .. row0 + R - 1 of the launch that draws
    with call number `call` (the device counter + 1) under `seed`"""
    rows = np.arange(row0, row0 + np.asarray(s).shape[0])
    xi = param_normals(seed, call, rows, dtype) if sd else None
    za = action_normals(seed, call, rows, dtype) if action_sd else None
    return forward_with_normals(P, s, sd, xi, action_sd, za, squares, dtype)


# ---------------------------------------------------------------- the noise-free 32-row tile's GEMMs
def split3(v):
    """fp32 array -> its (hi, mid, lo) bf16 pieces (sk_split.hpp split4), as fp64"""
    v = np.asarray(v, dtype=np.float32)
    hi = bf16_round(v)
    r1 = v - hi  # exact in fp32
    mid = bf16_round(r1)
    lo = bf16_round(r1 - mid)
    return hi.astype(np.float64), mid.astype(np.float64), lo.astype(np.float64)


# (x piece, w piece) of the six products mf6 keeps: 0 hi, 1 mid, 2 lo
SPLIT_PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


def split_gemm(x, W, products=SPLIT_PRODUCTS):
    """x W^T from bf16 pieces: the piece products in `products`, summed in fp64"""
    xs, ws = split3(x), split3(W)
    return sum(xs[i] @ ws[j].T for i, j in products)


def split_forward(P, s, products=SPLIT_PRODUCTS):
    """the noise-free forward with layers 1 and 2 on split_gemm (their inputs
    rounded to fp32, as the tile holds them), everything else in fp64"""
    Q = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}
    h = np.maximum(split_gemm(s, Q["l1.weight"], products) + Q["l1.bias"], 0)
    h = np.maximum(split_gemm(h, Q["l2.weight"], products) + Q["l2.bias"], 0)
    return np.tanh(h @ Q["l3.weight"].T + Q["l3.bias"])
