// C ABI, second part: the single-op entry points the op-level tests hold to fp64 emulations, and the micro-benchmarks of tools/.
// Every packed operand (Lin / NormW) comes out of the models' own WeightBuilder (struct Packed below), so an entry runs the packing,
// LayerNorm folding, weight scaling and kernel selection of the UNet / VAE, not a restatement of them.
#include "capi_internal.h"
#include <algorithm>
#include <cmath>

using namespace sdxl;

namespace {
__global__ void transpose_pad_kernel(const float* src, int lds_, int rows, int C, void* dst, int dt, int ldd) {
  // dst[c][r] = src[r][c]   (dst rows of ldd elements, caller zero-fills the padding)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows * C) return;
  const int r = i / C, c = i - (size_t)r * C;
  const float v = src[(size_t)r * lds_ + c];
  if (dt == DT_F16) reinterpret_cast<_Float16*>(dst)[(size_t)c * ldd + r] = (_Float16)v;
  else reinterpret_cast<float*>(dst)[(size_t)c * ldd + r] = v;
}
__global__ void causal_mask_kernel(float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n) return;
  const int r = i / n, c = i - r * n;
  out[i] = c > r ? -INFINITY : 0.f;
}

// one canonical (reference-layout fp32) parameter of an entry: device or host data, null for zeros; PK_EPS takes the host scalar
struct Operand { std::string name; std::vector<int> shape; int kind; const float* data = nullptr; float eps = 0.f; int ld = 0; };   // ld: row pitch of a [rows][cols] source (0: dense)
using Operands = std::vector<Operand>;
void add_linear(Operands& o, const std::string& n, int K, int N, const float* w, const float* b, int ld = 0) {
  o.push_back({n + ".weight", {K, N}, PK_LINEAR_W, w, 0.f, ld}); o.push_back({n + ".bias", {N}, PK_BIAS, b});
}
void add_conv(Operands& o, const std::string& n, int Cout, int Cin, int ksize, const float* w, const float* b) {
  o.push_back({n + ".weight", {Cout, Cin, ksize, ksize}, PK_CONV_W, w}); o.push_back({n + ".bias", {Cout}, PK_BIAS, b});
}
void add_norm(Operands& o, const std::string& n, int C, const float* gamma, const float* beta, float eps) {
  o.push_back({n + ".gamma", {C}, PK_GAMMA, gamma}); o.push_back({n + ".beta", {C}, PK_BETA, beta}); o.push_back({n + ".eps", {1}, PK_EPS, nullptr, eps});
}
// An entry packs a handful of operands lazily, in forms it chooses after this bound is taken: a coarse upper bound on what WeightBuilder can allocate for them
// (the models size their arenas by a layout pass instead).  Per matrix: padded weights (twice: the widest forms double K, the folded upsample phases hold
// 16/9 of a 3x3 kernel) + their fragment-order image + bias, column sums, plain-twin bias and the scalars; per vector its padded length.
size_t operand_bound(const std::vector<ParamSpec>& specs, int dt) {
  size_t total = 1 << 20;
  for (const ParamSpec& p : specs) {
    if (p.kind != PK_LINEAR_W && p.kind != PK_CONV_W) { total += round_up(p.numel(), 128) * sizeof(float) + 256; continue; }
    const size_t n = round_up(p.kind == PK_LINEAR_W ? p.shape[1] : p.shape[0], 128), k = round_up(p.numel() / (p.kind == PK_LINEAR_W ? p.shape[1] : p.shape[0]), 64);
    total += 2 * (n * k * dt_size(dt) + n * k * 2 + 3 * (n * 4 + 256) + 4 * 256);
  }
  return total;
}
// the parameters of an entry as a model holds them: spec list, flat device buffer, source, arena and the WeightBuilder over them
struct Packed {
  std::vector<ParamSpec> specs;
  Tmp tmp;
  FlatSource src;
  DeviceArena arena;
  WeightBuilder wb;
  Packed(const Operands& ops, int cdt, hipStream_t s)
      : specs(specs_of(ops)), src(stage(ops, specs, tmp, s), specs), wb(specs, src, reserved(arena, operand_bound(specs, cdt)), cdt, s) {}
  static std::vector<ParamSpec> specs_of(const Operands& ops) {
    std::vector<ParamSpec> v;
    for (const Operand& o : ops) v.push_back(ParamSpec{o.name, o.shape, o.kind, 0.f, 0.f});
    return v;
  }
  static const float* stage(const Operands& ops, const std::vector<ParamSpec>& specs, Tmp& tmp, hipStream_t s) {
    size_t total = 0;
    for (const ParamSpec& p : specs) total += p.numel();
    float* flat = (float*)tmp.get(total * sizeof(float)), *d = flat;
    for (size_t i = 0; i < ops.size(); ++i) {
      const Operand& o = ops[i];
      const size_t n = specs[i].numel(), cols = o.shape.back();
      if (o.kind == PK_EPS) SDXL_HIP(hipMemcpyAsync(d, &o.eps, sizeof(float), hipMemcpyHostToDevice, s));
      else if (!o.data) SDXL_HIP(hipMemsetAsync(d, 0, n * sizeof(float), s));
      else if (o.ld) SDXL_HIP(hipMemcpy2DAsync(d, cols * sizeof(float), o.data, (size_t)o.ld * sizeof(float), cols * sizeof(float), n / cols, hipMemcpyDefault, s));
      else SDXL_HIP(hipMemcpyAsync(d, o.data, n * sizeof(float), hipMemcpyDefault, s));
      d += n;
    }
    SDXL_HIP(hipStreamSynchronize(s));
    return flat;
  }
  static DeviceArena& reserved(DeviceArena& a, size_t bytes) { a.reserve(bytes); return a; }
};

// The f16 residual stream as the UNet's consumers meet it: it leaves its producer GEMM with per-64-column (mean, M2) statistics.  The
// producer here is x * I (exact; K % 128 == 0 puts it on the weights-in-registers kernel, pair-exchanged row statistics), so rows = f16(x).
struct F16Stream { void* rows; float* stat; };
F16Stream identity_producer(Exec& ex, Tmp& tmp, const float* x, int M, int K, hipStream_t s) {
  std::vector<float> eye((size_t)K * K, 0.f);
  for (int k = 0; k < K; ++k) eye[(size_t)k * K + k] = 1.0f;
  Packed id({{"eye.weight", {K, K}, PK_LINEAR_W, eye.data()}}, DT_F16, s);
  void* x16 = tmp.get((size_t)M * K * 2);
  F16Stream o{tmp.get((size_t)M * K * 2), (float*)tmp.get((size_t)M * (K / 64) * 2 * sizeof(float))};
  launch_copy_rows(x, DT_F32, K, x16, DT_F16, K, M, K, s);
  Epi e; e.stat_out = o.stat;
  run_linear(ex, id.wb.linear("eye"), Act(x16, K, DT_F16), M, Act(o.rows, K, DT_F16), e);
  SDXL_HIP(hipStreamSynchronize(s));      // (the identity's weights go with `id`)
  return o;
}
void transpose_pad(const float* src, int lds, int rows, int C, void* dst, int dt, int ldd, hipStream_t s) {
  hipLaunchKernelGGL(transpose_pad_kernel, dim3(((size_t)rows * C + 255) / 256), dim3(256), 0, s, src, lds, rows, C, dst, dt, ldd);
}
// V^T [B][C][vt_ld] (dt: f16 or fp32, zero key padding) of the fp32 values v [B][Nk][C]
void* stage_vt(Tmp& tmp, const float* v, int B, int Nk, int C, int dt, int vt_ld, hipStream_t s) {
  const size_t entry = (size_t)C * vt_ld * dt_size(dt);
  char* vt = (char*)tmp.get(B * entry);
  launch_fill_zero(vt, B * entry, s);
  for (int b = 0; b < B; ++b) transpose_pad(v + (size_t)b * Nk * C, C, Nk, C, vt + b * entry, dt, vt_ld, s);
  return vt;
}
// head-dim-64 (or one wide head) attention over dense rows of C channels, no mask
AttnParams attn_params(const void* q, const void* k, const void* vt, int vt_ld, void* o, int C, int dt, int B, int H, int Nq, int Nk, float scale = 0.125f) {
  AttnParams p{};
  p.Q = q; p.ldq = C; p.K = k; p.ldk = C; p.Vt = vt; p.vt_ld = vt_ld; p.O = o; p.ldo = C;
  p.dt = dt; p.B = B; p.H = H; p.Nq = Nq; p.Nk = Nk; p.scale = scale; p.mask = nullptr; p.ldmask = 0;
  return p;
}
// workspace + tickets of the cross-workgroup key split (what the UNet hands its self-attention calls)
void give_xsplit_ws(AttnParams& p, Tmp& tmp, hipStream_t s) {
  p.xws = (float*)tmp.get(attention_xsplit_ws_bytes(p.B, p.H, p.Nq) + 256);
  p.xcnt = (unsigned*)tmp.get(attention_xsplit_counters(p.B, p.H, p.Nq) * sizeof(unsigned) + 256);
  launch_fill_zero(p.xcnt, attention_xsplit_counters(p.B, p.H, p.Nq) * sizeof(unsigned), s);
}
// average milliseconds of fn(i), i = 0 .. iters - 1, after `warmup` calls of fn(0)
template <class F> float time_launches(hipStream_t s, int warmup, int iters, F fn) {
  for (int i = 0; i < warmup; ++i) fn(0);
  hipEvent_t a, b;
  SDXL_HIP(hipEventCreate(&a)); SDXL_HIP(hipEventCreate(&b));
  SDXL_HIP(hipEventRecord(a, s));
  for (int i = 0; i < iters; ++i) fn(i);
  SDXL_HIP(hipEventRecord(b, s));
  SDXL_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  SDXL_HIP(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  return ms / iters;
}
// A block of the autoencoder run the way Vae runs it (Vae's constructor and its two-pass execution): compute dtype of the mode with the stream in io_dt()
// (fp32 under the split-operand mode), a builder without fragment-order images, and an activation arena sized by a dry run of the block with the GroupNorm
// workspace of the batch at its head.  body(ex) allocates from ex.act and launches (helpers skip their launches on the dry pass).
void vae_block_dtypes(int dtype, int& cdt, int& sdt) {
  SDXL_REQUIRE(dtype == SDXL_DTYPE_F32 || dtype == SDXL_DTYPE_F16 || dtype == SDXL_DTYPE_F32_SPLIT,
               "the VAE block entries take SDXL_DTYPE_F32, SDXL_DTYPE_F16 or SDXL_DTYPE_F32_SPLIT");
  vae_dtype(dtype, cdt);
  sdt = cdt == DT_HL ? DT_F32 : cdt;
}
void vae_block_shape(int B, int C, int H, int W, int n_group, int cdt) {
  SDXL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (size_t)B * H * W * (size_t)(C > 0 ? C : 1) < ((size_t)1 << 31), "VAE block: B, H, W >= 1 and fewer than 2^31 elements");
  SDXL_REQUIRE(n_group >= 1 && n_group <= 256, "n_group out of range (1..256)");
  SDXL_REQUIRE(C > 0 && C % n_group == 0 && C % 8 == 0, "The number of channels must be divisible by the number of groups (and by 8)");
  SDXL_REQUIRE(cdt != DT_HL || C % 32 == 0, "SDXL_DTYPE_F32_SPLIT blocks need channel counts that are multiples of 32");
}
template <class F> void vae_block_run(DeviceArena& act, int cdt, int sdt, int B, int n_group, hipStream_t s, F body) {
  Exec ex; ex.s = s; ex.cdt = cdt; ex.sdt = sdt; ex.act = &act;
  for (int pass = 0; pass < 2; ++pass) {
    act.dry = ex.dry = pass == 0; act.off = 0; act.peak = 0;
    ex.gn_partial = (float*)act.alloc(groupnorm_workspace_floats(B, n_group) * sizeof(float));
    body(ex);
    if (pass == 0) act.reserve(act.peak + 4096);
  }
}
}  // namespace

extern "C" {

int sdxl_bench_igemm(sdxl_ctx* ctx, void* stream, int B, int H, int W, int Cin, int Cout, int ksize, int geglu, int iters,
                     float* avg_ms) {
  // times the implicit-GEMM kernel alone on seeded random f16 data: conv ksize x ksize (pad ksize/2) or, with ksize = 1,
  // a linear over B*H*W rows.  Epilogue: bias (+ GEGLU when geglu != 0).  Used by tools/igemm_sweep.py.
  API_BEGIN
  SDXL_REQUIRE(ctx && avg_ms && iters > 0, "bad argument");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  Tmp tmp;
  const int K = Cin * ksize * ksize;
  const size_t M = (size_t)B * H * W;
  float* wsrc = (float*)tmp.get((size_t)Cout * K * sizeof(float));
  float* bsrc = (float*)tmp.get((size_t)Cout * sizeof(float));
  float* xsrc = (float*)tmp.get(M * Cin * sizeof(float));
  void* xi = tmp.get(M * Cin * 2);
  void* yo = tmp.get(M * Cout * 2);
  launch_synth_fill(wsrc, (size_t)Cout * K, 0x1234, 3.4641f / std::sqrt((float)K), 0.f, s);
  launch_synth_fill(bsrc, Cout, 0x99, 0.1f, 0.f, s);
  launch_synth_fill(xsrc, M * Cin, 0x777, 3.4641f, 0.f, s);
  launch_copy_rows(xsrc, DT_F32, Cin, xi, DT_F16, Cin, (int)M, Cin, s);
  const bool ln_in = (geglu & 2) != 0, st_out = (geglu & 4) != 0, cold = (geglu & 8) != 0;
  geglu &= 1;
  Operands ops;
  if (ksize == 1) add_linear(ops, "w", K, Cout, wsrc, bsrc);   // [K][N] random == fine
  else add_conv(ops, "w", Cout, Cin, ksize, wsrc, bsrc);
  Packed pk(ops, DT_F16, s);
  Lin l = ksize == 1 ? pk.wb.linear("w", geglu != 0) : pk.wb.conv("w");
  Exec ex; ex.s = s; ex.cdt = DT_F16; ex.sdt = DT_F16;
  give_splitk_ws(ex, tmp, B, H * W, Cout, s);
  // cold mode: rotate through enough copies of the weight (> 256 MB Infinity Cache) that every launch streams it from HBM,
  // as in the model where each of the ~500 weights is touched once per step
  std::vector<const void*> wcopies(1, l.w), wfcopies(1, l.wf);
  if (cold) {
    const size_t wbytes = (size_t)l.Npad * l.Kpad * 2;
    const int nc = (int)std::min<size_t>(96, (size_t)(320u << 20) / wbytes + 1);
    for (int i = 1; i < nc; ++i)
      for (auto* img : {&wcopies, &wfcopies}) {
        void* c = img->front() ? tmp.get(wbytes) : nullptr;
        if (c) SDXL_HIP(hipMemcpyAsync(c, img->front(), wbytes, hipMemcpyDeviceToDevice, s));
        img->push_back(c);
      }
  }
  Epi e; e.act = geglu ? 1 : 0;
  if (ln_in) {   // timing of the LayerNorm-folded epilogue: plausible statistics (sum 0, sum^2 = 64 per slot), unit column sums
    SDXL_REQUIRE(ksize == 1 && Cin % 64 == 0, "ln bench needs a linear with K % 64 == 0");
    float* stat = (float*)tmp.get(M * (size_t)(Cin / 64) * 2 * sizeof(float));
    float* cs = (float*)tmp.get((size_t)l.Npad * sizeof(float));
    launch_synth_fill(stat, M * (size_t)(Cin / 64) * 2, 0x31, 0.5f, 64.0f, s);
    launch_synth_fill(cs, l.Npad, 0x32, 0.1f, 0.f, s);
    l.cs = cs; e.ln_stat = stat;
  }
  if (st_out) {
    SDXL_REQUIRE(!geglu && Cout % 64 == 0, "stat bench needs a plain N % 64 == 0 output");
    e.stat_out = (float*)tmp.get(M * (size_t)(Cout / 64) * 2 * sizeof(float));
  }
  const ConvGeom g{B, H, W, H, W, ksize, 1, ksize / 2, 0};
  const Act out(yo, geglu ? Cout / 2 : Cout, DT_F16);
  *avg_ms = time_launches(s, 3, iters, [&](int i) {
    l.w = wcopies[(size_t)i % wcopies.size()];
    l.wf = wfcopies[(size_t)i % wfcopies.size()];
    run_conv(ex, l, Act(xi, Cin, DT_F16), Cin, g, out, e);
  });
  API_END
}
int sdxl_bench_attention(sdxl_ctx* ctx, void* stream, int B, int H, int Nq, int Nk, int iters, float* avg_ms) {
  API_BEGIN
  SDXL_REQUIRE(ctx && avg_ms && iters > 0, "bad argument");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  Tmp tmp;
  const int C = H * 64, npad = (int)round_up(Nk, 64);
  float* src = (float*)tmp.get((size_t)B * std::max(Nq, npad) * C * sizeof(float));
  void* q = tmp.get((size_t)B * Nq * C * 2);
  void* k = tmp.get((size_t)B * Nk * C * 2);
  void* vt = tmp.get((size_t)B * C * npad * 2);
  void* o = tmp.get((size_t)B * Nq * C * 2);
  launch_synth_fill(src, (size_t)B * Nq * C, 0x51, 3.4641f, 0.f, s);
  launch_copy_rows(src, DT_F32, C, q, DT_F16, C, B * Nq, C, s);
  launch_synth_fill(src, (size_t)B * Nk * C, 0x52, 3.4641f, 0.f, s);
  launch_copy_rows(src, DT_F32, C, k, DT_F16, C, B * Nk, C, s);
  launch_synth_fill(src, (size_t)B * C * npad, 0x53, 3.4641f, 0.f, s);
  launch_copy_rows(src, DT_F32, npad, vt, DT_F16, npad, B * C, npad, s);   // random V^T (padding columns included: timing only)
  AttnParams p = attn_params(q, k, vt, npad, o, C, DT_F16, B, H, Nq, Nk);
  give_xsplit_ws(p, tmp, s);
  *avg_ms = time_launches(s, 3, iters, [&](int) { launch_attention_d64(p, s); });
  API_END
}

// ---------------------------------------------------------------------------------------------- attention op
int sdxl_qkv_attention(sdxl_ctx* ctx, void* stream, const float* q, const float* k, const float* v, const float* mask, int B,
                       int Nq, int Nk, int n_state, int n_head, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && q && k && v && out, "null argument");
  SDXL_REQUIRE(n_head > 0 && n_state % n_head == 0, "State size must be a multiple of head size");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  int cdt, sdt; no_mix(dtype); dtypes(dtype, cdt, sdt);
  const int d = n_state / n_head, npad = (int)round_up(Nk, 64);
  const size_t es = dt_size(cdt);
  const float scale = (float)(1.0 / std::sqrt((double)d));
  Tmp tmp;
  if (cdt == DT_HL) {
    // split-operand mode: Q / O stay fp32, K and V^T go through the HL16 format of the split GEMMs (attn_d64_hl_kernel)
    SDXL_REQUIRE(d == 64 && !mask, "sdxl_qkv_attention: the split-operand mode covers unmasked head-dim-64 attention");
    void* kh = tmp.get((size_t)B * Nk * n_state * 4);
    void* vth = tmp.get((size_t)B * n_state * npad * 4);
    launch_f32_to_hl(k, n_state, kh, n_state, (size_t)B * Nk, n_state, s);
    launch_f32_to_hl(stage_vt(tmp, v, B, Nk, n_state, DT_F32, npad, s), npad, vth, npad, (size_t)B * n_state, npad, s);
    const AttnParams p = attn_params(q, kh, vth, npad, out, n_state, DT_HL, B, n_head, Nq, Nk);
    SDXL_REQUIRE(launch_attention_d64_hl(p, s), "split-operand attention kernel refused an aligned shape");
  } else if (d == 64 || (d == 512 && cdt == DT_F16 && !mask)) {
    void* qd = tmp.get((size_t)B * Nq * n_state * es);
    void* kd = tmp.get((size_t)B * Nk * n_state * es);
    void* od = tmp.get((size_t)B * Nq * n_state * es);
    launch_copy_rows(q, DT_F32, n_state, qd, cdt, n_state, B * Nq, n_state, s);
    launch_copy_rows(k, DT_F32, n_state, kd, cdt, n_state, B * Nk, n_state, s);
    AttnParams p = attn_params(qd, kd, stage_vt(tmp, v, B, Nk, n_state, cdt, npad, s), npad, od, n_state, cdt, B, n_head, Nq, Nk, scale);
    p.mask = mask; p.ldmask = Nk;
    if (d == 64 && cdt == DT_F16 && !mask) give_xsplit_ws(p, tmp, s);
    if (d == 64) launch_attention_d64(p, s);
    else SDXL_REQUIRE(launch_attention_hd512(p, s), "wide-head attention kernel refused an aligned f16 shape");
    launch_copy_rows(od, cdt, n_state, out, DT_F32, n_state, B * Nq, n_state, s);
  } else {
    // generic head dim: QK^T GEMM -> row softmax -> PV GEMM per (batch, head)
    const int kt = cdt == DT_F16 ? 64 : 32;
    const int dpad = (int)round_up(d, kt), kpad = (int)round_up(Nk, kt);
    const int rows_k = (int)round_up(Nk, 128), rows_v = (int)round_up(d, 128);
    void* qh = tmp.get((size_t)Nq * dpad * es);
    void* kh = tmp.get((size_t)rows_k * dpad * es);
    void* vt = tmp.get((size_t)rows_v * kpad * es);
    float* S = (float*)tmp.get((size_t)Nq * Nk * sizeof(float));
    void* P = tmp.get((size_t)Nq * kpad * es);
    launch_fill_zero(qh, (size_t)Nq * dpad * es, s);
    launch_fill_zero(kh, (size_t)rows_k * dpad * es, s);
    launch_fill_zero(vt, (size_t)rows_v * kpad * es, s);
    Exec ex; ex.s = s; ex.cdt = cdt; ex.sdt = sdt;
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < n_head; ++h) {
        const float* qs = q + (size_t)b * Nq * n_state + h * d;
        const float* ks = k + (size_t)b * Nk * n_state + h * d;
        const float* vs = v + (size_t)b * Nk * n_state + h * d;
        launch_copy_rows(qs, DT_F32, n_state, qh, cdt, dpad, Nq, d, s);
        launch_copy_rows(ks, DT_F32, n_state, kh, cdt, dpad, Nk, d, s);
        transpose_pad(vs, n_state, Nk, d, vt, cdt, kpad, s);
        Lin lk; lk.w = kh; lk.N = Nk; lk.K = dpad; lk.Kpad = dpad; lk.Npad = rows_k; lk.cin = dpad;      // (activations as the "weight": nothing to pack)
        run_linear(ex, lk, Act(qh, dpad, cdt), Nq, Act(S, Nk, DT_F32));
        launch_softmax_rows(S, Nk, P, cdt, kpad, Nq, Nk, kpad, scale, mask, Nk, Nq, s);
        Lin lv; lv.w = vt; lv.N = d; lv.K = Nk; lv.Kpad = kpad; lv.Npad = rows_v; lv.cin = Nk;
        run_linear(ex, lv, Act(P, kpad, cdt), Nq, Act(out + (size_t)b * Nq * n_state + h * d, n_state, DT_F32));
      }
  }
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
int sdxl_attn_decoder_mask(sdxl_ctx* ctx, void* stream, int n, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && out && n > 0, "bad argument");
  use(ctx);
  hipLaunchKernelGGL(causal_mask_kernel, dim3((n * n + 255) / 256), dim3(256), 0, pick(ctx, stream), out, n);
  API_END
}

// ---------------------------------------------------------------------------------------------- norms, convolution, linear
int sdxl_group_norm(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, int B, int C, int HW,
                    int n_group, float eps, int silu, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && gamma && beta && out, "null argument");
  SDXL_REQUIRE(n_group > 0 && C % n_group == 0, "The number of channels must be divisible by the number of groups");
  SDXL_REQUIRE(C % 8 == 0 && n_group <= 256, "unsupported GroupNorm shape");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  int cdt, sdt; no_mix(dtype); dtypes(dtype, cdt, sdt); no_split(cdt, "sdxl_group_norm");
  Tmp tmp;
  void* xi = tmp.get((size_t)B * HW * C * dt_size(sdt));
  void* yo = tmp.get((size_t)B * HW * C * dt_size(cdt));
  float* part = (float*)tmp.get(groupnorm_workspace_floats(B, n_group) * sizeof(float));
  launch_nchw_to_nhwc(x, C * HW, xi, sdt, B, C, HW, C, 1.0f, s);
  GroupNormParams p{};
  p.X = xi; p.x_dt = sdt; p.ldx = C; p.Y = yo; p.y_dt = cdt; p.ldy = C; p.gamma = gamma; p.beta = beta; p.partial = part;
  p.B = B; p.HW = HW; p.C = C; p.G = n_group; p.eps = eps; p.silu = silu;
  launch_groupnorm(p, s);
  launch_nhwc_to_nchw(yo, cdt, C, out, B, C, HW, 1.0f, s);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
int sdxl_layer_norm(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, int rows, int C,
                    float eps, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && gamma && beta && out, "null argument");
  SDXL_REQUIRE(C % 8 == 0, "unsupported LayerNorm width");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  int cdt, sdt; no_mix(dtype); dtypes(dtype, cdt, sdt); no_split(cdt, "sdxl_layer_norm");
  Tmp tmp;
  void* xi = tmp.get((size_t)rows * C * dt_size(sdt));
  void* yo = tmp.get((size_t)rows * C * dt_size(cdt));
  launch_copy_rows(x, DT_F32, C, xi, sdt, C, rows, C, s);
  LayerNormParams p{};
  p.X = xi; p.x_dt = sdt; p.ldx = C; p.Y = yo; p.y_dt = cdt; p.ldy = C; p.gamma = gamma; p.beta = beta; p.rows = rows; p.C = C; p.eps = eps;
  launch_layernorm(p, s);
  launch_copy_rows(yo, cdt, C, out, DT_F32, C, rows, C, s);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
int sdxl_conv2d(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, int B, int Cin, int H,
                int W, int Cout, int ksize, int stride, int pad, int upsample, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && weight && out, "null argument");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  int cdt, sdt;
  if (dtype == SDXL_DTYPE_F32_SPLIT) { cdt = DT_HL; sdt = DT_HL; }   // split-operand GEMM as an operator (the VAE's precision): HL16 operands
  else { no_mix(dtype); dtypes(dtype, cdt, sdt); }
  SDXL_REQUIRE(cdt != DT_HL || Cin % 32 == 0, "SDXL_DTYPE_F32_SPLIT convolutions need Cin % 32 == 0");   // (the builder would pack such a layer fp32)
  const int Hs = upsample ? 2 * H : H, Ws = upsample ? 2 * W : W;
  const int Ho = (Hs + 2 * pad - ksize) / stride + 1, Wo = (Ws + 2 * pad - ksize) / stride + 1;
  Operands ops;
  add_conv(ops, "conv", Cout, Cin, ksize, weight, bias);
  Packed pk(ops, cdt, s);
  const Lin l = pk.wb.conv("conv");
  Tmp tmp;
  void* xi = tmp.get((size_t)B * H * W * Cin * dt_size(sdt));
  float* yo = (float*)tmp.get((size_t)B * Ho * Wo * Cout * sizeof(float));
  Act xa(xi, Cin, sdt);
  if (cdt == DT_HL) {      // range-safe conversion, as the models convert their fp32 stream tensors (hl_operand)
    float* x32 = (float*)tmp.get((size_t)B * H * W * Cin * sizeof(float));
    float* sc = (float*)tmp.get(hl_scale_floats(B) * sizeof(float));
    launch_nchw_to_nhwc(x, Cin * H * W, x32, DT_F32, B, Cin, H * W, Cin, 1.0f, s);
    launch_f32_to_hl_scaled(x32, Cin, xi, Cin, (size_t)B * H * W, Cin, sc, s, B);      // one factor per batch entry, as the models' hl_operand
    xa.a_scale = hl_scale_inv(sc, B); xa.a_scale_n = B;
  } else launch_nchw_to_nhwc(x, Cin * H * W, xi, sdt, B, Cin, H * W, Cin, 1.0f, s);
  Exec ex; ex.s = s; ex.cdt = cdt; ex.sdt = sdt;
  give_splitk_ws(ex, tmp, B, Ho * Wo, Cout, s);
  run_conv(ex, l, xa, Cin, ConvGeom{B, H, W, Ho, Wo, ksize, stride, pad, upsample ? 1 : 0}, Act(yo, Cout, DT_F32));
  launch_nhwc_to_nchw(yo, DT_F32, Cout, out, B, Cout, Ho * Wo, 1.0f, s);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
// nearest-2x upsample + 3x3 convolution (pad 1) the way the f16 UNet and the split-operand VAE decoder run it: the weights folded into four 2x2-tap
// phase matrices at pack time (WeightBuilder::conv fold_up), one phase-ordered launch where the shape has one (*folded reports it), else the gather form
int sdxl_conv2d_upsample_folded(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, int B, int Cin, int H, int W,
                                int Cout, int dtype, int* folded, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && weight && out, "null argument");
  SDXL_REQUIRE(dtype == SDXL_DTYPE_F16 || dtype == SDXL_DTYPE_F32_SPLIT, "the folded upsample convolution exists in the f16 and the split-operand engines");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  const int cdt = dtype == SDXL_DTYPE_F16 ? DT_F16 : DT_HL, sdt = cdt;
  SDXL_REQUIRE(Cin % (cdt == DT_HL ? 32 : 64) == 0, "the folded upsample convolution needs whole k-tiles per tap (Cin % 64, split-operand: Cin % 32)");
  Operands ops;
  add_conv(ops, "conv", Cout, Cin, 3, weight, bias);
  Packed pk(ops, cdt, s);
  const Lin l = pk.wb.conv("conv", true);
  Tmp tmp;
  const size_t rows = (size_t)B * H * W;
  void* xi = tmp.get(rows * Cin * dt_size(sdt));
  float* yo = (float*)tmp.get(4 * rows * Cout * sizeof(float));
  Act xa(xi, Cin, sdt);
  if (cdt == DT_HL) {      // (as sdxl_conv2d: one range factor per batch entry)
    float* x32 = (float*)tmp.get(rows * Cin * sizeof(float));
    float* sc = (float*)tmp.get(hl_scale_floats(B) * sizeof(float));
    launch_nchw_to_nhwc(x, Cin * H * W, x32, DT_F32, B, Cin, H * W, Cin, 1.0f, s);
    launch_f32_to_hl_scaled(x32, Cin, xi, Cin, rows, Cin, sc, s, B);
    xa.a_scale = hl_scale_inv(sc, B); xa.a_scale_n = B;
  } else launch_nchw_to_nhwc(x, Cin * H * W, xi, sdt, B, Cin, H * W, Cin, 1.0f, s);
  Exec ex; ex.s = s; ex.cdt = cdt; ex.sdt = sdt;
  give_splitk_ws(ex, tmp, B, 4 * H * W, Cout, s);
  Epi e; e.fold = true;
  bool took = false; e.fold_done = &took;
  run_conv(ex, l, xa, Cin, ConvGeom{B, H, W, 2 * H, 2 * W, 3, 1, 1, 1}, Act(yo, Cout, DT_F32), e);
  if (folded) *folded = took ? 1 : 0;
  launch_nhwc_to_nchw(yo, DT_F32, Cout, out, B, Cout, 4 * H * W, 1.0f, s);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
int sdxl_linear(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, int M, int K, int N,
                int geglu, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && weight && out, "null argument");
  SDXL_REQUIRE(!geglu || (N % 32 == 0), "GEGLU width must be a multiple of 32");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  int cdt, sdt;
  if (dtype == SDXL_DTYPE_F32_SPLIT) { cdt = DT_HL; sdt = DT_HL; }   // split-operand GEMM as an operator: HL16 operands (incl. the GEGLU epilogue)
  else { no_mix(dtype); dtypes(dtype, cdt, sdt); }
  SDXL_REQUIRE(cdt != DT_HL || K % 32 == 0, "SDXL_DTYPE_F32_SPLIT linear layers need K % 32 == 0");   // (the builder would pack such a layer fp32)
  Operands ops;
  add_linear(ops, "lin", K, N, weight, bias);
  Packed pk(ops, cdt, s);
  const Lin l = pk.wb.linear("lin", geglu != 0);
  Tmp tmp;
  void* xi = tmp.get((size_t)M * K * dt_size(sdt));
  Act xa(xi, K, sdt);
  if (cdt == DT_HL) {      // range-safe conversion, as the models convert their fp32 stream tensors (hl_operand)
    float* sc = (float*)tmp.get(hl_scale_floats(1) * sizeof(float));
    launch_f32_to_hl_scaled(x, K, xi, K, (size_t)M, K, sc, s, 1);
    xa.a_scale = hl_scale_inv(sc, 1);
  } else launch_copy_rows(x, DT_F32, K, xi, sdt, K, M, K, s);
  Exec ex; ex.s = s; ex.cdt = cdt; ex.sdt = sdt;
  give_splitk_ws(ex, tmp, 1, M, N, s);
  Epi e; e.act = geglu ? 1 : 0;
  run_linear(ex, l, xa, M, Act(out, geglu ? N / 2 : N, DT_F32), e);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
// the conditioning path's small-M linear (UNet::run / UNet::set_context: time and label MLPs, the hoisted lin_embed(silu(emb))): the weight packed as
// the UNet of that dtype packs its GEMV weights (gemv_weight_dt), the launcher's row chunking included; x / yadd / out are used in place (dense rows)
int sdxl_gemv(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, const float* yadd, int Bm, int K, int N,
              int silu_in, int silu_out, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && weight && out, "null argument");
  SDXL_REQUIRE(Bm >= 1 && K >= 1 && N >= 1, "gemv: Bm, K, N must be >= 1");
  SDXL_REQUIRE(dtype == SDXL_DTYPE_F32 || dtype == SDXL_DTYPE_F16 || dtype == SDXL_DTYPE_F32_SPLIT,
               "sdxl_gemv takes SDXL_DTYPE_F32, SDXL_DTYPE_F16 or SDXL_DTYPE_F32_SPLIT");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  const int cdt = dtype == SDXL_DTYPE_F16 ? DT_F16 : dtype == SDXL_DTYPE_F32_SPLIT ? DT_HL : DT_F32;
  Operands ops;
  add_linear(ops, "lin", K, N, weight, bias);
  Packed pk(ops, cdt, s);
  const Lin l = pk.wb.linear("lin", false, gemv_weight_dt(cdt));
  GemvParams p{};
  p.X = x; p.ldx = K; p.W = l.w; p.w_dt = l.dt >= 0 ? l.dt : cdt; p.Kpad = l.Kpad; p.bias = bias ? l.b : nullptr;
  p.Y = out; p.ldy = N; p.Yadd = yadd; p.Bm = Bm; p.N = l.N; p.K = l.K;
  p.silu_in = silu_in != 0; p.silu_out = silu_out != 0;
  (void)hipGetLastError();      // (every call before this one was checked: what is read below belongs to the GEMV launches)
  launch_gemv(p, s);
  SDXL_HIP(hipGetLastError());
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
// timestep_embedding (unet/mod.rs:21-39) of n fp32 timesteps: out[i] = [cos(t[i] f) | sin(t[i] f)], f_j = exp(-ln(10000) j / (dim / 2))
int sdxl_timestep_embedding(sdxl_ctx* ctx, void* stream, const float* t, int n, int dim, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && t && out, "null argument");
  SDXL_REQUIRE(n >= 1 && dim >= 2 && dim % 2 == 0, "timestep_embedding: n >= 1 and an even dim >= 2");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  (void)hipGetLastError();
  launch_timestep_embedding(t, 1, out, n, dim, s);
  SDXL_HIP(hipGetLastError());
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
// the per-step add of the ControlNet skip residuals (UNet::run behind the middle block) on caller buffers: the table is checked on the host, uploaded,
// and the one launch walks it.  src[i * K + k]; step_idx_dev == nullptr: scales_dev is one device scalar (B == 0, K == 1); else the trajectory form,
// scales_dev[(*step_idx_dev * K + k) * 8 + entry of the row]
static void skip_add_impl(sdxl_ctx* ctx, void* stream, int n_segments, void* const* dst, const int64_t* dst_ld, const void* const* src, int K,
                          const int64_t* rows, const int32_t* C, int B, const float* scales_dev, const int32_t* step_idx_dev, int dtype) {
  static_assert(SDXL_MAX_CONTROLS == kSkipMaxSources, "one source per control net");
  if (!ctx || !dst || !dst_ld || !src || !rows || !C || !scales_dev) throw InvalidArgumentError("skip residual add: null argument");
  if (n_segments < 1 || n_segments > 16) throw InvalidArgumentError("skip residual add: n_segments must be in 1..16");
  if (K < 1 || K > SDXL_MAX_CONTROLS) throw InvalidArgumentError("skip residual add: the number of sources K must be in 1..4");
  if (step_idx_dev && B < 1) throw InvalidArgumentError("skip residual add: B must be in 1..8");      // (0 would name the one-scalar form to skip_table_check)
  if (dtype != SDXL_DTYPE_F32 && dtype != SDXL_DTYPE_F16) throw InvalidArgumentError("skip residual add: the dtype must be SDXL_DTYPE_F32 or SDXL_DTYPE_F16");
  const int dt = dtype == SDXL_DTYPE_F16 ? DT_F16 : DT_F32;
  SkipSeg table[16];
  for (int i = 0; i < n_segments; ++i) {
    if (rows[i] < 0 || rows[i] > 0x7fffffff || dst_ld[i] < 0) throw InvalidArgumentError("skip residual add: rows must be in 0..2^31-1 and dst_ld >= C");
    table[i] = SkipSeg{dst[i], {nullptr, nullptr, nullptr, nullptr}, (long long)dst_ld[i], (int)rows[i], (int)C[i], 0ull};
    for (int k = 0; k < K; ++k) table[i].src[k] = src[(size_t)i * K + k];
  }
  unsigned long long total = 0;
  if (const char* bad = skip_table_check(table, n_segments, K, B, dt, &total)) throw InvalidArgumentError(bad);
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  Tmp tmp;
  SkipSeg* table_dev = (SkipSeg*)tmp.get(sizeof(table));
  SDXL_HIP(hipMemcpyAsync(table_dev, table, n_segments * sizeof(SkipSeg), hipMemcpyHostToDevice, s));
  (void)hipGetLastError();
  launch_skip_add(table_dev, n_segments, K, total, scales_dev, step_idx_dev, B, dt, s);
  SDXL_HIP(hipGetLastError());
  SDXL_HIP(hipStreamSynchronize(s));
}
int sdxl_skip_residual_add(sdxl_ctx* ctx, void* stream, int n_segments, void* const* dst, const int64_t* dst_ld, const void* const* src,
                           const int64_t* rows, const int32_t* C, const float* scale_dev, int dtype) {
  API_BEGIN
  skip_add_impl(ctx, stream, n_segments, dst, dst_ld, src, 1, rows, C, 0, scale_dev, nullptr, dtype);
  API_END
}
int sdxl_skip_residual_add_steps(sdxl_ctx* ctx, void* stream, int n_segments, void* const* dst, const int64_t* dst_ld, const void* const* src,
                                 const int64_t* rows, const int32_t* C, int B, const float* scales_dev, const int32_t* step_idx_dev, int dtype) {
  return sdxl_skip_residual_add_steps_multi(ctx, stream, n_segments, dst, dst_ld, src, 1, rows, C, B, scales_dev, step_idx_dev, dtype);
}
int sdxl_skip_residual_add_steps_multi(sdxl_ctx* ctx, void* stream, int n_segments, void* const* dst, const int64_t* dst_ld, const void* const* src, int K,
                                       const int64_t* rows, const int32_t* C, int B, const float* scales_dev, const int32_t* step_idx_dev, int dtype) {
  API_BEGIN
  if (!step_idx_dev) throw InvalidArgumentError("skip residual add: null argument");
  skip_add_impl(ctx, stream, n_segments, dst, dst_ld, src, K, rows, C, B, scales_dev, step_idx_dev, dtype);
  API_END
}
int sdxl_layer_norm_linear(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, float eps,
                           const float* weight, const float* bias, int M, int K, int N, int geglu, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && gamma && beta && weight && out, "null argument");
  SDXL_REQUIRE(!geglu || (N % 32 == 0), "GEGLU width must be a multiple of 32");
  SDXL_REQUIRE(K % 64 == 0, "LayerNorm width must be a multiple of 64");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  int cdt, sdt; no_mix(dtype); dtypes(dtype, cdt, sdt); no_split(cdt, "sdxl_layer_norm_linear");
  Operands ops;
  add_linear(ops, "lin", K, N, weight, bias);
  add_norm(ops, "norm", K, gamma, beta, eps);
  Packed pk(ops, cdt, s);
  Tmp tmp;
  Exec ex; ex.s = s; ex.cdt = cdt; ex.sdt = sdt;
  const Act o(out, geglu ? N / 2 : N, DT_F32);
  Epi e; e.act = geglu ? 1 : 0;
  if (cdt == DT_F16 && sdt == DT_F16) {
    // f16 mode of the UNet: the consumer applies the LayerNorm in its epilogue, from the statistics the stream's producer left
    const F16Stream xs = identity_producer(ex, tmp, x, M, K, s);
    e.ln_stat = xs.stat;
    Proj d; d.names = {"lin"}; d.geglu = geglu != 0; d.ln = LN_FOLD; d.norm = "norm";
    run_linear(ex, pk.wb.pack(d), Act(xs.rows, K, DT_F16), M, o, e);
  } else {
    const NormW n = pk.wb.norm("norm");
    void* xi = tmp.get((size_t)M * K * dt_size(sdt));
    launch_copy_rows(x, DT_F32, K, xi, sdt, K, M, K, s);
    void* ln = tmp.get((size_t)M * K * dt_size(cdt));
    run_layernorm(ex, n, Act(xi, K, sdt), M, Act(ln, K, cdt));
    run_linear(ex, pk.wb.linear("lin", geglu != 0), Act(ln, K, cdt), M, o, e);
  }
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}

int sdxl_ln_query_cross_attention(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, float eps,
                                  const float* wq, const float* k, const float* v, int B, int Nq, int Nk, int C, int fused,
                                  float* out) {
  // attn2 of a transformer block up to (not including) the output projection: LayerNorm -> query projection (no bias) ->
  // qkv_attention over the projected context, 64 channels per head.  f16 engine only (the UNet's production mode); fused != 0
  // runs the attention inside the projection's epilogue (Nk <= 96; fused == 1 also 97 .. 384 keys where C % 128 == 0: the long form of the
  // weights-in-registers launch), fused == 0 as projection + attention kernel; fused == 2: the epilogue at split precision
  // (context, q and P as (hi, lo) f16 pairs: the SDXL_DTYPE_F32_SPLIT_MIX_F16W form).
  API_BEGIN
  SDXL_REQUIRE(ctx && x && gamma && beta && wq && k && v && out, "null argument");
  SDXL_REQUIRE(C % 64 == 0 && B >= 1 && Nq >= 1 && Nk >= 1, "State size must be a multiple of head size");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  const int M = B * Nq, vt_ld = (int)round_up(Nk, 64), H = C / 64;
  // (fused == 1 runs on fragment-order weights: up to 384 keys where the weights-in-registers form takes the width; the other forms up to 96)
  SDXL_REQUIRE(!fused || igemm_xattn_ok(DT_F16, DT_F16, M, C, C, Nq, Nk, igemm_launch_knobs(), fused != 2 && fused != 3), "fused cross-attention: unsupported shape");
  Operands ops;
  add_linear(ops, "lin", C, C, wq, nullptr);
  add_norm(ops, "norm", C, gamma, beta, eps);
  Packed pk(ops, DT_F16, s);
  Tmp tmp;
  Exec ex; ex.s = s; ex.cdt = DT_F16; ex.sdt = DT_F16;
  // beta W is folded into the packed bias; attn2.query has none of its own, so fold with beta as given (zero beta -> no bias)
  Proj d; d.names = {"lin"}; d.ln = LN_FOLD; d.norm = "norm"; d.wfrag_folded = true;
  const Lin l = pk.wb.pack(d);
  const F16Stream xs = identity_producer(ex, tmp, x, M, C, s);
  const Act xi(xs.rows, C, DT_F16);
  void* od = tmp.get((size_t)M * C * 2);
  Epi e; e.ln_stat = xs.stat; e.rpb = Nq;
  if (fused == 3) {
    // the un-fused twin of fused == 2: fp32 q out of the f16 projection, HL16 context, the stand-alone split-operand attention kernel writing f16 rows
    float* q32 = (float*)tmp.get((size_t)M * C * 4);
    run_linear(ex, l, xi, M, Act(q32, C, DT_F32), e);
    void* khl = tmp.get((size_t)B * Nk * C * 4);
    void* vhl = tmp.get((size_t)B * C * vt_ld * 4);
    launch_f32_to_hl(k, C, khl, C, (size_t)B * Nk, C, s);
    launch_f32_to_hl(stage_vt(tmp, v, B, Nk, C, DT_F32, vt_ld, s), vt_ld, vhl, vt_ld, (size_t)B * C, vt_ld, s);
    AttnParams p = attn_params(q32, khl, vhl, vt_ld, od, C, DT_HL, B, H, Nq, Nk);
    p.q_dt = DT_F32; p.o_dt = DT_F16;
    SDXL_REQUIRE(launch_attention_d64_hl(p, s), "split-operand attention: unsupported shape");
  } else if (fused == 2) {
    // split precision (IgemmParams::xa_k_lo): the fp32 context as (hi, lo) f16 pairs, q and P split inside the epilogue -- three MFMAs per product
    void* kh = tmp.get((size_t)B * Nk * C * 2); void* kl = tmp.get((size_t)B * Nk * C * 2);
    void* vh = tmp.get((size_t)B * C * vt_ld * 2); void* vl = tmp.get((size_t)B * C * vt_ld * 2);
    launch_f32_to_f16_pair(k, C, kh, kl, C, (size_t)B * Nk, C, s);
    launch_f32_to_f16_pair((const float*)stage_vt(tmp, v, B, Nk, C, DT_F32, vt_ld, s), vt_ld, vh, vl, vt_ld, (size_t)B * C, vt_ld, s);
    void* xa = tmp.get(xattn_pack_bytes(B, C, Nk)); void* xal = tmp.get(xattn_pack_bytes(B, C, Nk));
    launch_xattn_pack(kh, vh, xa, B, C, Nk, vt_ld, s);
    launch_xattn_pack(kl, vl, xal, B, C, Nk, vt_ld, s);
    e.xa_k = xa; e.xa_k_lo = xal; e.xa_nctx = Nk; e.xa_scale = 0.125f;
    run_linear(ex, l, xi, M, Act(od, C, DT_F16), e);
  } else {
    // context keys [B][Nk][C] and V^T [B][C][vt_ld] (zero key padding), f16
    void* kd = tmp.get((size_t)B * Nk * C * 2);
    launch_copy_rows(k, DT_F32, C, kd, DT_F16, C, B * Nk, C, s);
    void* vt = stage_vt(tmp, v, B, Nk, C, DT_F16, vt_ld, s);
    if (fused) {
      void* xa = tmp.get(xattn_pack_bytes(B, C, Nk));
      launch_xattn_pack(kd, vt, xa, B, C, Nk, vt_ld, s);
      e.xa_k = xa; e.xa_nctx = Nk; e.xa_scale = 0.125f;
      run_linear(ex, l, xi, M, Act(od, C, DT_F16), e);
    } else {
      void* qd = tmp.get((size_t)M * C * 2);
      run_linear(ex, l, xi, M, Act(qd, C, DT_F16), e);
      launch_attention_d64(attn_params(qd, kd, vt, vt_ld, od, C, DT_F16, B, H, Nq, Nk), s);
    }
  }
  launch_copy_rows(od, DT_F16, C, out, DT_F32, C, M, C, s);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}

int sdxl_transformer_projection(sdxl_ctx* ctx, void* stream, int B, int rows_per_entry, int C, const float* a, const float* wp, const float* bp,
                                const float* r, int Kp, int producer_form, const float* gamma, const float* beta, float eps, const float* w,
                                const float* b, int N, int proj, int form, int shadow, float* t_out, float* out, int* shadow_taken) {
  // one LayerNorm-fed projection of a split-operand UNet's transformer block in a named form (plan_transformer), through the code
  // UNet::spatial_transformer runs: WeightBuilder::pack, alloc_ln_operands, want_ln_shadow, ln_input.  The producer (an out-projection / FF-out) adds into the
  // fp32 stream t in place and, with `shadow`, is asked for the shadow of LayerNorm(t) exactly as the UNet asks it.
  API_BEGIN
  SDXL_REQUIRE(ctx && r && gamma && beta && w && out, "null argument");
  if (B < 1 || rows_per_entry < 1 || C < 32 || C % 32 != 0 || N < 1) return fail(SDXL_ERR_INVALID, "transformer projection: B, rows >= 1, C % 32 == 0");
  if (proj < SDXL_PROJ_QKV || proj > SDXL_PROJ_GEGLU || form < SDXL_FORM_NATIVE || form > SDXL_FORM_X2 || producer_form > SDXL_FORM_X2)
    return fail(SDXL_ERR_INVALID, "transformer projection: unknown projection or form");
  const LinForm f = (LinForm)form, pf = producer_form < 0 ? LF_NATIVE : (LinForm)producer_form;
  const bool geglu = proj == SDXL_PROJ_GEGLU, has_p = producer_form >= 0;
  const int parts = proj == SDXL_PROJ_QKV ? 3 : 1;
  // what plan_transformer lets each form take (anything else would compute wrong numbers, not fail)
  if (N % (32 * parts) != 0) return fail(SDXL_ERR_INVALID, "transformer projection: N % 32 == 0 per projection");
  if ((f == LF_F16_WHILO || f == LF_F16_AHILO) && !geglu) return fail(SDXL_ERR_INVALID, "transformer projection: the (hi | lo) forms are GEGLU forms");
  if (f == LF_X2 && (N / parts % 128 != 0 || (geglu && N % 640 != 0))) return fail(SDXL_ERR_INVALID, "transformer projection: X2 needs N % 128 == 0 (GEGLU: N % 640 == 0)");
  if (f == LF_X2 && proj == SDXL_PROJ_QKV && !shadow) return fail(SDXL_ERR_INVALID, "transformer projection: the X2 QKV projection exists only as a shadow-form pair");
  if (has_p && (!a || !wp || Kp < 32 || Kp % 32 != 0)) return fail(SDXL_ERR_INVALID, "transformer projection: a producer needs its operand, its weight and K % 32 == 0");
  if (has_p && pf == LF_X2 && (Kp % 32 != 0 || C % 128 != 0)) return fail(SDXL_ERR_INVALID, "transformer projection: an X2 producer needs K % 32 == 0 and C % 128 == 0");
  if (has_p && (pf == LF_F16_WHILO || pf == LF_F16_AHILO)) return fail(SDXL_ERR_INVALID, "transformer projection: producers run NATIVE, F16 or X2");
  if (shadow && (!has_p || pf == LF_NATIVE || C % 64 != 0 || !(f == LF_F16 || f == LF_F16_AHILO || f == LF_X2)))
    return fail(SDXL_ERR_INVALID, "transformer projection: a shadow needs an F16 / X2 producer, C % 64 == 0 and an F16, AHILO or X2 consumer");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  const size_t M = (size_t)B * rows_per_entry;
  const int Np = N / parts;
  // parameters: producer, LayerNorm, consumer (QKV: three projections fused along N, as the UNet packs attn1.query / key / value)
  Operands ops;
  if (has_p) add_linear(ops, "prod", Kp, C, wp, bp);
  add_norm(ops, "norm", C, gamma, beta, eps);
  std::vector<std::string> names, wnames;
  for (int i = 0; i < parts; ++i) {      // columns [i Np, (i + 1) Np) of w
    names.push_back("p" + std::to_string(i)); wnames.push_back(names.back() + ".weight");
    add_linear(ops, names.back(), C, Np, w + (size_t)i * Np, b ? b + (size_t)i * Np : nullptr, N);
  }
  Packed pk(ops, DT_HL, s);
  WeightBuilder& wb = pk.wb;
  // the forms that pack the parameter's values as f16 need f16 values (the UNet's create-time guard); LF_F16 rounds them -- that is its class
  if ((f == LF_F16_AHILO || f == LF_X2) && !wb.all_f16_exact(wnames)) return fail(SDXL_ERR_INVALID, "transformer projection: AHILO / X2 need f16-valued weights");
  if (has_p && pf == LF_X2 && !wb.all_f16_exact({"prod.weight"})) return fail(SDXL_ERR_INVALID, "transformer projection: an X2 producer needs f16-valued weights");
  const NormW n = wb.norm("norm");
  Lin sh;
  Proj d; d.names = names; d.geglu = geglu; d.form = f;
  if (shadow) { d.ln = LN_SHADOW; d.norm = "norm"; d.shadow = &sh; }
  const Lin plain = wb.pack(d);
  Proj dp; dp.names = {"prod"}; dp.form = pf;
  const Lin lp = has_p ? wb.pack(dp) : Lin();
  // the UNet's plan for this one projection: its form (+ shadow twin) in its slot
  StPlan pl;
  LinForm& slot = proj == SDXL_PROJ_QKV ? pl.qkv : proj == SDXL_PROJ_QUERY ? pl.q2 : pl.geglu;
  bool& slot_sh = proj == SDXL_PROJ_QKV ? pl.qkv_sh : proj == SDXL_PROJ_QUERY ? pl.q2_sh : pl.geglu_sh;
  slot = f; slot_sh = shadow != 0;
  Tmp tmp;
  DeviceArena act;
  act.reserve(M * (size_t)C * 40 + M * (size_t)N * 8 + (size_t)(has_p ? M * Kp * 4 : 0) + (1 << 20));
  Exec ex; ex.s = s; ex.cdt = DT_HL; ex.sdt = DT_F32; ex.act = &act;
  ex.splitk_ws_bytes = igemm_splitk_ws_bytes(B, std::max(rows_per_entry, 1024), std::max(N, 1536));      // (the UNet's own, larger than this shape's: give_splitk_ws sizes f16 engines)
  ex.splitk_ws = (float*)tmp.get(ex.splitk_ws_bytes);
  ex.splitk_cnt = (unsigned*)tmp.get(kSplitkCounters * sizeof(unsigned));
  SDXL_HIP(hipMemsetAsync(ex.splitk_cnt, 0, kSplitkCounters * sizeof(unsigned), s));
  const Act t = ex.alloc(M, C, DT_F32);
  launch_copy_rows(r, DT_F32, C, t.p, DT_F32, C, (int)M, C, s);
  const Act ln = ex.alloc(M, C, DT_HL);
  LnOperands lo;
  alloc_ln_operands(ex, pl, M, C, ln, lo);
  const int cls = proj == SDXL_PROJ_QKV ? DM_QKV : proj == SDXL_PROJ_QUERY ? DM_XATTN : DM_GEGLU;
  if (has_p) {
    // the producer's operand as spatial_transformer hands it over: f16 rows (an f16 out-projection), or the un-scaled HL16 rows the attention writes
    Act pa = ex.alloc(M, Kp, pf == LF_F16 ? DT_F16 : DT_HL);
    if (pf == LF_F16) launch_copy_rows(a, DT_F32, Kp, pa.p, DT_F16, Kp, (int)M, Kp, s);
    else launch_f32_to_hl(a, Kp, pa.p, Kp, M, Kp, s);
    Epi e; e.R = t; e.rpb = rows_per_entry; e.cls = proj == SDXL_PROJ_QKV ? DM_FF : DM_OUT;
    if (pf != LF_NATIVE) want_ln_shadow(lo, e, shadow != 0, f, n);
    run_linear(ex, lp, x2_operand(pf, pa), (int)M, t, e);
  }
  const LnIn in = ln_input(ex, lo, plain, sh, f, n, t, cls);
  if (shadow_taken) *shadow_taken = in.stat ? 1 : 0;
  // the consumer's output rows as the UNet stores them: the GEGLU output HL16 (f16, widened, on small token counts); an f16 QKV projection
  // writes f16 for the f16 self-attention, an f16 query projection fp32 q; the others HL16 where the attention takes it (else fp32).
  // (The QKV projection's V^T transposition is not modelled: all 3 C columns are stored as rows.)
  const int No = geglu ? N / 2 : N;
  const bool hl_direct = rows_per_entry % 8 == 0 && (2 * C) % 128 == 0;
  const bool widen = geglu && geglu_widened(f, in, M);
  const int odt = geglu ? (widen ? DT_F16 : DT_HL) : f == LF_F16 ? (proj == SDXL_PROJ_QKV ? DT_F16 : DT_F32) : hl_direct ? DT_HL : DT_F32;
  Act o = ex.alloc(M, No, odt);
  Epi e; e.act = geglu ? 1 : 0; e.ln_stat = in.stat; e.cls = cls;
  if (proj == SDXL_PROJ_QKV || in.stat || (proj == SDXL_PROJ_QUERY && f == LF_F16)) e.rpb = rows_per_entry;     // (as the UNet's launches select their kernel)
  run_linear(ex, *in.w, in.a, (int)M, o, e);
  if (widen) {
    const Act o2 = ex.alloc(M, No, DT_HL);
    launch_f16_to_hl(o.p, o.ld, o2.p, o2.ld, M, No, s);
    o = o2;
  }
  launch_copy_rows(o.p, o.dt, o.ld, out, DT_F32, No, (int)M, No, s);
  if (t_out) launch_copy_rows(t.p, DT_F32, C, t_out, DT_F32, C, (int)M, C, s);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}

int sdxl_conv2d_group_norm(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, const float* residual,
                           const float* gamma, const float* beta, float eps, int B, int Cin, int H, int W, int Cout, int n_group,
                           int silu, int fused, int* fused_taken, float* out) {
  // conv3x3 (pad 1, + optional residual) followed by GroupNorm(+SiLU) -- the conv -> norm pairs of ResBlock::forward
  // (unet/mod.rs:1082-1106) and of the SpatialTransformer entry (:820-845) on the f16 engine.  fused != 0 asks the convolution's
  // epilogue for the GroupNorm statistics (no statistics pass); *fused_taken reports whether the selected kernel provided them.
  API_BEGIN
  SDXL_REQUIRE(ctx && x && weight && gamma && beta && out, "null argument");
  SDXL_REQUIRE(n_group > 0 && Cout % n_group == 0, "The number of channels must be divisible by the number of groups");
  SDXL_REQUIRE(Cout % 8 == 0 && n_group <= 256, "unsupported GroupNorm shape");
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  const int cdt = DT_F16, HW = H * W;
  Operands ops;
  add_conv(ops, "conv", Cout, Cin, 3, weight, bias);
  add_norm(ops, "norm", Cout, gamma, beta, eps);
  Packed pk(ops, cdt, s);
  const Lin l = pk.wb.conv("conv");
  const NormW n = pk.wb.norm("norm");
  Tmp tmp;
  void* xi = tmp.get((size_t)B * HW * Cin * 2);
  void* hh = tmp.get((size_t)B * HW * Cout * 2);
  void* yo = tmp.get((size_t)B * HW * Cout * 2);
  void* ri = residual ? tmp.get((size_t)B * HW * Cout * 2) : nullptr;
  float* part = (float*)tmp.get(groupnorm_workspace_floats(B, n_group) * sizeof(float));
  launch_nchw_to_nhwc(x, Cin * HW, xi, cdt, B, Cin, HW, Cin, 1.0f, s);
  if (residual) launch_nchw_to_nhwc(residual, Cout * HW, ri, cdt, B, Cout, HW, Cout, 1.0f, s);
  Exec ex; ex.s = s; ex.cdt = cdt; ex.sdt = cdt; ex.gn_partial = part;
  give_splitk_ws(ex, tmp, B, HW, Cout, s);
  Act h(hh, Cout, cdt);
  Epi e;
  if (residual) e.R = Act(ri, Cout, cdt);
  if (fused && HW % 256 == 0) e.gn_part = (float*)tmp.get((size_t)B * HW / 256 * Cout * 2 * sizeof(float));
  const bool took = run_conv(ex, l, Act(xi, Cin, cdt), Cin, ConvGeom{B, H, W, H, W, 3, 1, 1, 0}, h, e);
  if (took) { h.gn_part = e.gn_part; h.gn_rt = HW / 256; }
  if (fused_taken) *fused_taken = took ? 1 : 0;
  run_groupnorm(ex, n, h, B, HW, Act(yo, Cout, cdt), silu != 0, n_group);
  launch_nhwc_to_nchw(yo, cdt, Cout, out, B, Cout, HW, 1.0f, s);
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}

// ---------------------------------------------------------------------------------------------- VAE blocks
// ConvSelfAttentionBlock::forward (autoencoder/mod.rs:550-586) through vae_attn_block, the code Vae::mid runs: GroupNorm, 1x1 q / k / v, one head of C
// channels (f16 with C = 512: the flash kernel; else score GEMM -> row softmax -> P V GEMM in passes of 8192 queries), proj_out + residual
int sdxl_vae_attn_block(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, float eps, const float* wq, const float* bq,
                        const float* wk, const float* bk, const float* wv, const float* bv, const float* wo, const float* bo, int B, int C, int H, int W,
                        int n_group, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && gamma && beta && wq && wk && wv && wo && out, "null argument");
  int cdt, sdt; vae_block_dtypes(dtype, cdt, sdt);
  vae_block_shape(B, C, H, W, n_group, cdt);
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  Operands ops;
  add_norm(ops, "attn.norm", C, gamma, beta, eps);
  add_conv(ops, "attn.q", C, C, 1, wq, bq); add_conv(ops, "attn.k", C, C, 1, wk, bk); add_conv(ops, "attn.v", C, C, 1, wv, bv);
  add_conv(ops, "attn.proj_out", C, C, 1, wo, bo);
  Packed pk(ops, cdt, s);
  pk.wb.wfrag = false;
  VaeMidW w; w.C = C;
  vae_load_attn(pk.wb, "attn", w);
  DeviceArena act;
  const int HW = H * W;
  vae_block_run(act, cdt, sdt, B, n_group, s, [&](Exec& ex) {
    Act y = ex.alloc((size_t)B * HW, C, sdt);
    if (!ex.dry) launch_nchw_to_nhwc(x, C * HW, y.p, sdt, B, C, HW, C, 1.0f, s);
    vae_attn_block(ex, w, y, B, H, W, n_group);
    if (!ex.dry) launch_nhwc_to_nchw(y.p, sdt, C, out, B, C, HW, 1.0f, s);
  });
  SDXL_HIP(hipGetLastError());
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}
// ResnetBlock::forward (autoencoder/mod.rs:500-516) through vae_res_block, the code every block of Vae runs: GroupNorm + SiLU, conv 3x3, GroupNorm + SiLU,
// conv 3x3 + shortcut (x, or the 1x1 nin_shortcut of x -- split-operand mode: on the HL16 copy scaled per batch entry from the maxima norm1's statistics pass leaves)
int sdxl_vae_res_block(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma1, const float* beta1, float eps1, const float* w1, const float* b1,
                       const float* gamma2, const float* beta2, float eps2, const float* w2, const float* b2, const float* w_nin, const float* b_nin, int B,
                       int Cin, int Cout, int H, int W, int n_group, int dtype, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && x && gamma1 && beta1 && w1 && gamma2 && beta2 && w2 && out, "null argument");
  SDXL_REQUIRE(w_nin || Cin == Cout, "a ResnetBlock that changes the channel count needs its nin_shortcut weight");
  SDXL_REQUIRE(w_nin || !b_nin, "nin_shortcut bias without its weight");
  int cdt, sdt; vae_block_dtypes(dtype, cdt, sdt);
  vae_block_shape(B, Cin, H, W, n_group, cdt);
  vae_block_shape(B, Cout, H, W, n_group, cdt);
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  Operands ops;
  add_norm(ops, "res.norm1", Cin, gamma1, beta1, eps1);
  add_conv(ops, "res.conv1", Cout, Cin, 3, w1, b1);
  add_norm(ops, "res.norm2", Cout, gamma2, beta2, eps2);
  add_conv(ops, "res.conv2", Cout, Cout, 3, w2, b2);
  if (w_nin) add_conv(ops, "res.nin_shortcut", Cout, Cin, 1, w_nin, b_nin);
  Packed pk(ops, cdt, s);
  pk.wb.wfrag = false;
  const VaeResW w = vae_load_res(pk.wb, "res", Cin, Cout);
  DeviceArena act;
  const int HW = H * W;
  vae_block_run(act, cdt, sdt, B, n_group, s, [&](Exec& ex) {
    Act xi = ex.alloc((size_t)B * HW, Cin, sdt), yo = ex.alloc((size_t)B * HW, Cout, sdt);
    if (!ex.dry) launch_nchw_to_nhwc(x, Cin * HW, xi.p, sdt, B, Cin, HW, Cin, 1.0f, s);
    vae_res_block(ex, w, xi, B, H, W, yo, n_group);
    if (!ex.dry) launch_nhwc_to_nchw(yo.p, sdt, Cout, out, B, Cout, HW, 1.0f, s);
  });
  SDXL_HIP(hipGetLastError());
  SDXL_HIP(hipStreamSynchronize(s));
  API_END
}

// the create-time adapter merge on one resident tensor, through the source the models are built through (LoraSource: staging of host / device
// arrays, the merge kernel, the optional f16 rounding)
int sdxl_lora_merge(sdxl_ctx* ctx, void* stream, float* w_dev, int rows, int cols, const float* left, const float* right, int rank, float scale,
                    int flags) {
  if (!ctx || !w_dev) return fail(SDXL_ERR_INVALID, "null argument");
  if (rows < 1 || cols < 1) return fail(SDXL_ERR_INVALID, "lora_merge: rows, cols must be >= 1");
  if (flags & ~SDXL_LORA_ROUND_F16) return fail(SDXL_ERR_INVALID, "lora: unknown flag bits (SDXL_LORA_ROUND_F16)");
  const std::vector<ParamSpec> specs{ParamSpec{"w", {rows, cols}, PK_LINEAR_W, 0.f, 0.f}};
  LoraEntry e; e.param_index = 0; e.rank = rank; e.left = left; e.right = right; e.scale = scale;
  const std::string bad = lora_check(specs, &e, 1);
  if (!bad.empty()) return fail(SDXL_ERR_INVALID, bad);
  API_BEGIN
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  struct Resident : WeightSource { void fetch(const ParamSpec&, size_t, float*, hipStream_t) override {} } resident;      // the tensor is where fetch() would put it
  LoraSource src(resident, specs, &e, 1, flags);
  src.fetch(specs[0], 0, w_dev, s);
  API_END
}

}  // extern "C"
