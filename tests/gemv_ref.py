"""fp64 references, derived error bounds and an fp32-order CPU emulation of the UNet's conditioning path kernels (csrc/elementwise.hip):
gemv_kernel behind launch_gemv (time / label embedding MLPs, the hoisted lin_embed(silu(emb)) of the ResBlocks) and temb_kernel (the sinusoidal
timestep embedding).  Plain numpy; no GPU, no engine.

What the bounds are made of (nothing here is fitted to what a kernel returns):
  gemv: every lane of a wavefront adds at most ceil(K / (64 CE)) * CE <= K / 64 + CE products into one fp32 accumulator, six shuffle adds join the
        lanes, bias and yadd are two more adds, expf inside SiLU is a few ulps: at most (K / 64 + 16) roundings of 2^-24 relative to the sum of
        the magnitudes that were added.  SiLU on the way out scales an incoming error by |silu'| <= 1.1 and rounds its own result (4 ulps).
  temb: a = t * exp(j * coef): the rounding of j * coef (|j coef| 2^-24 relative to a), 1-ulp expf, the product, then 2-ulp cosf / sinf of an
        argument that is off by |a| (|j coef| + 4) 2^-24 (|cos'|, |sin'| <= 1).
"""
import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32

# defects gemv_emulate can plant (test_cpu_gemv_ref.py shows each one leaves the bound on the shapes where it changes anything)
DEFECTS = ("drop_last_product", "skip_partial_iter", "yadd_no_offset", "x_no_offset", "skip_silu_in", "skip_silu_out", "shift_out")
TAIL_DEFECTS = ("drop_last_product", "skip_partial_iter")


def silu64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


def silu32(v):
    """silu_f of elementwise.hip in fp32: x / (1 + expf(-x))"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore"):
        return (v / (np.float32(1.0) + np.exp(-v))).astype(np.float32)


def f16_rne(w):
    """fp32 -> f16 round-to-nearest-even -> fp64 (the packing's conversion, pinned by test_linear_conversion_weight_side_is_rne)"""
    return np.asarray(w, np.float32).astype(np.float16).astype(np.float64)


def ce_of(f16_weights):
    """weights per 16-byte piece: 8 f16 or 4 fp32"""
    return 8 if f16_weights else 4


def staged_k(K, f16_weights):
    """Kx of the kernel: K rounded up to one wavefront step of 64 * CE elements"""
    step = 64 * ce_of(f16_weights)
    return (K + step - 1) // step * step


def rows_per_launch(K, f16_weights):
    """launch_gemv: min(8, 64 KiB / bytes of one staged row); 0 = the launcher refuses K"""
    return min(8, (64 * 1024) // (staged_k(K, f16_weights) * 4))


def gemv_ref(x, w, bias, yadd, silu_in, silu_out, f16_weights):
    """(y, bound) per element, fp64: y = silu_out?(sum_k s_k w_k + bias) + yadd, s = silu(x) with silu_in; w rounded to f16 first with f16_weights.
    bound = (K / 64 + 16) 2^-24 (sum_k |s_k| |w_k| + |bias| + |yadd|); with silu_out the sum-and-bias part x 1.1, + 4 * 2^-24 |y|."""
    x = np.asarray(x, np.float64)
    K, N = w.shape
    wq = f16_rne(w) if f16_weights else np.asarray(w, np.float64)
    s = silu64(x) if silu_in else x
    b = np.zeros(N) if bias is None else np.asarray(bias, np.float64)
    pre = s @ wq + b
    mag = np.abs(s) @ np.abs(wq) + np.abs(b)
    u = (K / 64.0 + 16.0) * U
    y = silu64(pre) if silu_out else pre
    bound = (1.1 if silu_out else 1.0) * u * mag
    if yadd is not None:
        ya = np.asarray(yadd, np.float64)
        y = y + ya
        bound = bound + u * np.abs(ya)
    if silu_out:
        bound = bound + 4.0 * U * np.abs(y)
    return y, bound


def gemv_emulate(x, w, bias, yadd, silu_in, silu_out, f16_weights, defect=None):
    """gemv_kernel + launch_gemv in fp32 on the CPU, in the kernel's order: rows in chunks of rows_per_launch; per chunk the inputs (SiLU applied) staged
    in a zero-padded row of Kx; lane l of a wavefront walks the 16-byte pieces k0 = l CE, l CE + 64 CE, ... adding 4-term partial sums
    ((p0 + p1) + p2) + p3 into its accumulator; xor tree over the 64 lanes (32, 16, ..., 1); + bias, SiLU, + yadd.  Every product and sum is
    rounded on its own (the compiler may fuse some into FMAs on the device: fewer roundings, never more).
    defect: one of DEFECTS --
      drop_last_product  the product of element K - 1 is left out
      skip_partial_iter  the last k-iteration is not run when it is a partial one (K % (64 CE) != 0)
      yadd_no_offset     launches after the first read Yadd from row 0 (the launcher forgets the row offset)
      x_no_offset        the same for X
      skip_silu_in / skip_silu_out   the flag is ignored
      shift_out          column n receives the value of column n - 1 (cyclic)"""
    assert defect is None or defect in DEFECTS, defect
    f32 = np.float32
    x = np.asarray(x, f32)
    Bm, K = x.shape
    N = w.shape[1]
    CE, Kx, rpl = ce_of(f16_weights), staged_k(K, f16_weights), rows_per_launch(K, f16_weights)
    if rpl < 1:
        raise ValueError("gemv: K does not fit the 64 KiB input staging buffer")
    iters = Kx // (64 * CE)
    if defect == "skip_partial_iter" and K % (64 * CE) != 0:
        iters -= 1
    wp = np.zeros((N, Kx), f32)      # packed rows [N][Kpad], zero padding (read up to Kx here: the staged inputs are zero there as well)
    wp[:, :K] = (f16_rne(w).astype(f32) if f16_weights else np.asarray(w, f32)).T
    if defect == "drop_last_product":
        wp[:, K - 1] = 0.0
    wv = wp.reshape(N, Kx // (64 * CE), 64, CE // 4, 4)
    out = np.empty((Bm, N), f32)
    for b0 in range(0, Bm, rpl):
        bm = min(rpl, Bm - b0)
        xs = x[0:bm] if (defect == "x_no_offset" and b0) else x[b0:b0 + bm]
        gx = np.zeros((bm, Kx), f32)
        gx[:, :K] = silu32(xs) if (silu_in and defect != "skip_silu_in") else xs
        gv = gx.reshape(bm, 1, Kx // (64 * CE), 64, CE // 4, 4)
        acc = np.zeros((bm, N, 64), f32)
        for it in range(iters):
            for j in range(CE // 4):
                p = gv[:, :, it, :, j, :] * wv[None, :, it, :, j, :]      # [bm, N, 64, 4]
                acc = acc + (((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, lanes ^ o]
        v = acc[:, :, 0]
        if bias is not None:
            v = v + np.asarray(bias, f32)[None, :]
        if silu_out and defect != "skip_silu_out":
            v = silu32(v)
        if yadd is not None:
            ya = np.asarray(yadd, f32)
            v = v + (ya[0:bm] if (defect == "yadd_no_offset" and b0) else ya[b0:b0 + bm])
        out[b0:b0 + bm] = v
    if defect == "shift_out":
        out = np.roll(out, 1, axis=1)
    return out


def defect_applies(defect, K, Bm, has_yadd, silu_in, silu_out, f16_weights):
    """whether the defect changes anything the kernel computes for this launch (a chunk defect needs a second launch, ...)"""
    chunks = -(-Bm // rows_per_launch(K, f16_weights))
    return {"drop_last_product": True, "shift_out": True,
            "skip_partial_iter": K % (64 * ce_of(f16_weights)) != 0,
            "yadd_no_offset": has_yadd and chunks > 1, "x_no_offset": chunks > 1,
            "skip_silu_in": bool(silu_in), "skip_silu_out": bool(silu_out)}[defect]


# ---------------------------------------------------------------------------------------------------------------- the cases both test files run
# (name, K, N, Bm, flags): flags out of "b" bias, "a" yadd, "i" silu_in, "o" silu_out
GEMV_CASES = [
    ("tiny_idle_lanes", 64, 256, 2, ""),
    ("k_and_n_tails", 20, 3, 3, "b"),
    ("time_lin1_b1", 320, 1280, 1, "bo"),
    ("time_lin1_b2", 320, 1280, 2, "bo"),
    ("time_lin1_b8", 320, 1280, 8, "bo"),
    ("time_lin2_b2", 1280, 1280, 2, "ba"),
    ("time_lin2_b8", 1280, 1280, 8, "ba"),
    ("lin_embed_cols4", 1280, 8192, 2, "bi"),
    ("lin_embed_cols4_partial_block", 1280, 8200, 2, "bi"),
    ("label_base_b5", 2816, 256, 5, "bo"),
    ("label_base_b6", 2816, 256, 6, "bo"),
    ("label_base_b8", 2816, 256, 8, "bo"),
    ("label_refiner_b7", 2560, 256, 7, "bo"),
    ("chunks_of_8", 64, 64, 9, ""),
    ("staging_limit", 16384, 8, 2, ""),
    ("all_flags_null_bias_two_launches", 2816, 256, 8, "aio"),
]


def make_case(K, N, Bm, flags, f16_weights, seed=0):
    """seeded operands of a case: x ~ N(0, 1), w ~ N(0, 1 / K) (unit-size outputs, so SiLU sees both of its regimes), bias, yadd ~ N(0, 1).
    The last K % (64 CE) elements of x and w -- what a partial last k-iteration covers -- are 3 x larger, and element K - 1 of x is at least 8:
    an error in the tail is far larger than the rounding the bound allows."""
    rng = np.random.default_rng([seed, K, N, Bm])
    x = rng.standard_normal((Bm, K))
    w = rng.standard_normal((K, N)) / np.sqrt(K)
    tail = K % (64 * ce_of(f16_weights))
    if tail:
        x[:, K - tail:] *= 3.0
        w[K - tail:, :] *= 3.0
    else:
        w[K - 1, :] *= 3.0
    x[:, K - 1] = 8.0 * (1.0 + np.abs(rng.standard_normal(Bm)))
    bias = rng.standard_normal(N).astype(np.float32) if "b" in flags else None
    yadd = rng.standard_normal((Bm, N)).astype(np.float32) if "a" in flags else None
    return dict(x=x.astype(np.float32), w=w.astype(np.float32), bias=bias, yadd=yadd, silu_in="i" in flags, silu_out="o" in flags,
                f16_weights=bool(f16_weights))


# ---------------------------------------------------------------------------------------------------------------- timestep embedding
TEMB_T = [0.0, 1.0, 123.456, 250.0, 999.0, 500.0, 37.0, 981.0]
TEMB_DIMS = (64, 320, 384)


def temb_coef(dim):
    """-ln(10000) / half rounded to fp32, as temb_kernel and the reference (an f64 scalar turned into an f32 element) have it"""
    return float(np.float32(-9.210340371976184 / float(dim // 2)))


def temb_ref(t, dim):
    """(out [n, dim], bound) in fp64: [cos(t f) | sin(t f)], f_j = exp(j coef); t are the fp32 timesteps the kernel reads.
    bound = |a| (|j coef| + 4) 2^-24 + 2^-22, a = t f_j (the same for the cos and the sin column of j)"""
    half = dim // 2
    t = np.asarray(t, np.float32).astype(np.float64).reshape(-1)
    j = np.arange(half, dtype=np.float64)
    jc = j * temb_coef(dim)
    a = t[:, None] * np.exp(jc)[None, :]
    bound = np.abs(a) * (np.abs(jc)[None, :] + 4.0) * U + 2.0 ** -22
    return np.concatenate([np.cos(a), np.sin(a)], axis=1), np.concatenate([bound, bound], axis=1)


def temb_emulate(t, dim, defect=None):
    """temb_kernel in numpy fp32.  defect: "swap" (sin | cos), "dim_for_half" (coef over dim instead of dim / 2), "j_plus_1" (frequency index off by one)"""
    f32 = np.float32
    half = dim // 2
    t = np.asarray(t, f32).reshape(-1)
    coef = f32(-9.210340371976184 / float(dim if defect == "dim_for_half" else half))
    j = np.arange(half, dtype=f32) + f32(1.0 if defect == "j_plus_1" else 0.0)
    f = np.exp((j * coef).astype(f32)).astype(f32)
    a = (t[:, None] * f[None, :]).astype(f32)
    c, s = np.cos(a).astype(f32), np.sin(a).astype(f32)
    return np.concatenate([s, c] if defect == "swap" else [c, s], axis=1)
