// SDXL UNet forward on MI355X -- the sampling loop's hot path (reference UNet::forward, unet/mod.rs:450-492).
//
// Design (not a translation of the burn module tree):
//   * NHWC / token-major everywhere, so ResBlock convs, the SpatialTransformer's linears and attention share one
//     activation layout and the reference's NCHW<->[B,N,C] transposes (unet/mod.rs:827-829,837-841) disappear.
//   * torch.cat of the skip connections (:484) is eliminated: every input block writes its output straight into the
//     channel slice [C_x, C_x+C_skip) of the concat buffer its matching output block will read, and the previous
//     output block writes the [0, C_x) slice.
//   * nearest-2x upsample (:744-749) is an index >>1 inside the conv's gather; the time-embedding add (:1092), the
//     residual adds (:1098-1102, :887-889, :843) and GEGLU (:944-955) live in GEMM epilogues.
//   * everything that is constant over a trajectory is hoisted out of the step: cross-attention K / V^T projections of
//     the 70 transformer blocks and the label-embedding MLP are computed once per prompt (set_context).
//   * the 17+ per-ResBlock lin_embed(silu(emb)) GEMVs (:1088-1089) are one GEMV over a concatenated weight.
//   * static shapes -> bump-allocated activation arena with scoped reuse (working set stays inside the 256 MB
//     Infinity Cache) -> stable addresses -> the whole forward is captured once into a hipGraph and replayed.
#include "engine.h"

#include <atomic>
#include <cmath>
#include <cstring>

namespace sdxl {

namespace {
ResBlockW load_res(WeightBuilder& wb, const std::string& p, int cin, int cout, std::vector<std::string>& emb_names,
                   int& emb_off) {
  ResBlockW r;
  r.cin = cin; r.cout = cout;
  r.norm_in = wb.norm(p + ".norm_in");
  r.conv_in = wb.conv(p + ".conv_in");
  r.norm_out = wb.norm(p + ".norm_out");
  r.conv_out = wb.conv(p + ".conv_out");
  r.has_skip = wb.has(p + ".skip_connection.weight");
  if (r.has_skip) r.skip = wb.conv(p + ".skip_connection");
  r.emb_off = emb_off;
  emb_names.push_back(p + ".lin_embed");
  emb_off += cout;
  return r;
}
// parameter names of a transformer block's projections (suffixes of "<transformer>.blocks.<j>")
const std::vector<std::string> kQkv = {".attn1.query", ".attn1.key", ".attn1.value"};
const char* const kOut1 = ".attn1.out", *const kQ2 = ".attn2.query", *const kOut2 = ".attn2.out", *const kGeglu = ".mlp.geglu.proj", *const kFf = ".mlp.lin";

// the forms of transformer `p`'s projections for MixClass bits `mix` on compute dtype `cdt` (all blocks of a transformer share their shapes)
StPlan plan_transformer(int mix, int cdt, const std::vector<ParamSpec>& specs, const std::string& p) {
  StPlan s;
  if (cdt == DT_F16) s.xattn = XA_F16;
  auto shape = [&](const char* proj) -> const std::vector<int>* {
    const std::string n = p + ".blocks.0" + proj + ".weight";
    for (const ParamSpec& ps : specs) if (ps.name == n) return &ps.shape;
    return nullptr;
  };
  if (cdt != DT_HL || !shape(kQ2)) return s;
  auto fits = [&](const char* proj, int k, int n) { const std::vector<int>& sh = *shape(proj); return sh[0] % k == 0 && sh[1] % n == 0; };
  const bool ln_sh = (mix & MIX_LN_SHADOW) != 0, x2 = (mix & MIX_LINEAR_F16X2) != 0;
  const bool xattn_f16 = (mix & MIX_OUT2_F16) && (mix & MIX_XATTN_F16);
  // MIX_LINEAR_F16X2: a projection that stays fp32-class (its A operand an HL16 tensor) runs on the f16 kernels over the weight packed twice in the HL16 interleave
  auto x2_ok = [&](const char* proj) { return x2 && fits(proj, 32, 128); };
  // MIX_LN_SHADOW: the projections behind a LayerNorm also exist in the shadow form (same packed matrix, cs = gamma W, b = beta W + bias): where the
  // producer of the stream left the shadow f16(x o gamma) and the row statistics, the LayerNorm launch is skipped (spatial_transformer)
  if (mix & MIX_QKV_F16) { s.qkv = LF_F16; s.qkv_sh = ln_sh; }
  else if (ln_sh && x2 && fits(kQkv[0].c_str(), 64, 128)) { s.qkv = LF_X2; s.qkv_sh = true; }     // (the plain twin reads the LayerNorm launch's HL16 output)
  s.out1 = (mix & MIX_OUT1_F16) ? LF_F16 : x2_ok(kOut1) ? LF_X2 : LF_NATIVE;
  if ((mix & MIX_Q2_F16) || xattn_f16) { s.q2 = LF_F16; s.q2_sh = ln_sh && !xattn_f16; }
  else if (x2_ok(kQ2)) { s.q2 = LF_X2; s.q2_sh = ln_sh && fits(kQ2, 64, 1); }
  s.out2 = (mix & MIX_OUT2_F16) ? LF_F16 : x2_ok(kOut2) ? LF_X2 : LF_NATIVE;
  if (mix & MIX_GEGLU_F16) {
    const bool k32 = fits(kGeglu, 32, 1);
    if ((mix & MIX_GEGLU_AHILO) && k32) { s.geglu = LF_F16_AHILO; s.geglu_sh = ln_sh && fits(kGeglu, 64, 1); }   // (the shadow carries both halves)
    else if (ln_sh) { s.geglu = LF_F16; s.geglu_sh = true; }
    else s.geglu = (mix & MIX_GEGLU_HILO) && k32 ? LF_F16_WHILO : LF_F16;
  } else if (x2 && fits(kGeglu, 32, 640)) { s.geglu = LF_X2; s.geglu_sh = ln_sh && fits(kGeglu, 64, 1); }    // (K = 2 C on the f16 wide-tile kernel)
  s.ff = (mix & MIX_FF_F16) ? LF_F16 : x2_ok(kFf) ? LF_X2 : LF_NATIVE;
  s.attn_f16 = ((mix & MIX_ATTN_F16) || s.qkv == LF_F16) && shape(kQ2)->at(0) % 16 == 0;
  SDXL_REQUIRE(s.out1 != LF_F16 || s.attn_f16, "mixed mode: an f16 out-projection reads the f16 self-attention's output");
  // the split-precision epilogue writes the out-projection's operand: f16 rows for an f16 one, HL16 rows behind the X2 query projection
  if (xattn_f16) s.xattn = XA_F16;
  else if ((mix & MIX_XATTN_SPLIT) && ((s.q2 == LF_F16 && s.out2 == LF_F16) || (s.q2 == LF_X2 && s.out2 != LF_F16))) s.xattn = XA_SPLIT;
  return s;
}
// the weights of block `q` that plan `s` packs as f16 values (what the create-time guard checks)
void f16_valued_weights(const StPlan& s, const std::string& q, std::vector<std::string>& names) {
  auto add = [&](LinForm f, const char* proj) { if (packs_f16_values(f)) names.push_back(q + proj + ".weight"); };
  for (const std::string& n : kQkv) add(s.qkv, n.c_str());
  add(s.out1, kOut1); add(s.q2, kQ2); add(s.out2, kOut2); add(s.geglu, kGeglu); add(s.ff, kFf);
}
STW load_st(WeightBuilder& wb, const std::string& p, int C, int heads, int depth, bool fuse_ln, const StPlan& plan) {
  STW s;
  s.C = C; s.heads = heads; s.plan = plan;
  s.norm = wb.norm(p + ".norm");
  s.proj_in = wb.linear(p + ".proj_in");
  for (int j = 0; j < depth; ++j) {
    const std::string q = p + ".blocks." + std::to_string(j);
    const std::vector<std::string> qkv = {q + kQkv[0], q + kQkv[1], q + kQkv[2]};
    TBlockW t;
    // a projection in its planned form; behind LayerNorm `norm`: folded (f16 engine), or with its shadow twin `sh` where the plan has one
    auto proj = [&](LinForm f, const std::vector<std::string>& names, bool geglu = false, const char* norm = nullptr, Lin* sh = nullptr, bool xattn_query = false) {
      Proj d; d.names = names; d.geglu = geglu; d.form = f;
      if (norm && (fuse_ln || sh)) { d.ln = fuse_ln ? LN_FOLD : LN_SHADOW; d.norm = q + norm; d.shadow = sh; d.wfrag_folded = xattn_query; }
      return wb.pack(d);
    };
    // f16 engine: the three LayerNorms of TransformerBlock::forward (unet/mod.rs:885-891) are folded into the projections that
    // consume them; their row statistics come out of the epilogue of the GEMM that produced the residual stream
    if (!fuse_ln) t.n1 = wb.norm(q + ".norm1");
    t.qkv = proj(plan.qkv, qkv, false, ".norm1", plan.qkv_sh ? &t.qkv_sh : nullptr);
    t.out1 = proj(plan.out1, {q + kOut1});
    if (!fuse_ln) t.n2 = wb.norm(q + ".norm2");
    t.q2 = proj(plan.q2, {q + kQ2}, false, ".norm2", plan.q2_sh ? &t.q2_sh : nullptr, true);
    t.kv2 = wb.fused_linear({q + ".attn2.key", q + ".attn2.value"});
    t.out2 = proj(plan.out2, {q + kOut2});
    if (!fuse_ln) t.n3 = wb.norm(q + ".norm3");
    t.geglu = proj(plan.geglu, {q + kGeglu}, true, ".norm3", plan.geglu_sh ? &t.geglu_sh : nullptr);
    t.ff = proj(plan.ff, {q + kFf});
    s.blocks.push_back(t);
  }
  s.proj_out = wb.linear(p + ".proj_out");
  return s;
}
void gemv(Exec& ex, const Lin& w, const float* x, int ldx, float* y, int ldy, int Bm, bool silu_in, bool silu_out,
          const float* yadd = nullptr) {
  if (ex.dry) return;
  GemvParams p{};
  p.X = x; p.ldx = ldx; p.W = w.w; p.w_dt = w.dt >= 0 ? w.dt : ex.cdt; p.Kpad = w.Kpad; p.bias = w.b;
  p.Y = y; p.ldy = ldy; p.Yadd = yadd; p.Bm = Bm; p.N = w.N; p.K = w.K;
  p.silu_in = silu_in; p.silu_out = silu_out;
  if (ex.prof) ex.prof->begin(Profiler::OTHER, 2.0 * Bm * (double)w.N * w.K, ex.s);
  launch_gemv(p, ex.s);
  if (ex.prof) ex.prof->end(ex.s);
}
void attention(Exec& ex, const Act& q, const Act& k, const void* vt, int vt_ld, const Act& o, int B, int H, int Nq,
               int Nk, int tag = 0) {
  if (ex.dry) return;
  AttnParams p{};
  p.Q = q.p; p.ldq = q.ld; p.K = k.p; p.ldk = k.ld; p.Vt = vt; p.vt_ld = vt_ld; p.O = o.p; p.ldo = o.ld;
  // (the split-operand mode runs the attention on fp32 tensors: q / k / V^T / o all carry q's dtype)
  p.dt = q.dt; p.B = B; p.H = H; p.Nq = Nq; p.Nk = Nk; p.scale = 0.125f; p.mask = nullptr; p.ldmask = 0;
  if (Nq == Nk) { p.xws = ex.attn_xws; p.xcnt = ex.attn_xcnt; }      // self-attention: room for the cross-workgroup key split (sized for it in ensure_plan)
  if (ex.prof) ex.prof->begin(Profiler::ATTENTION, 4.0 * B * H * (double)Nq * Nk * 64, ex.s, Nq, Nk, B * H, 0, tag ? tag : (Nq == Nk ? DM_ATTN : DM_XATTN));
  launch_attention_d64(p, ex.s);
  {
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) throw Error(std::string("attention launch failed (") + hipGetErrorString(le) + "): Nq=" + std::to_string(Nq) + " Nk=" + std::to_string(Nk) + " dt=" + std::to_string(p.dt));
  }
  if (ex.prof) ex.prof->end(ex.s);
}
Epi tag_epi(int cls) { Epi e; e.cls = cls; return e; }      // plain epilogue carrying only the launch's class label
// hl_demote: lo halves of an HL16 operand := 0 when its consumer's class is demoted (no-op otherwise / for other dtypes)
void demote_lo(Exec& ex, int cls, const Act& a, size_t rows, int C) {
  if (ex.dry || !(ex.demote & cls) || a.dt != DT_HL) return;
  launch_hl_zero_lo(a.p, a.ld, rows, C, ex.s);
}
Act hl_op(Exec& ex, const Lin& w, const Act& x, size_t rows, int C, int cls, int nb, float* have_max = nullptr) {      // hl_operand + the demotion of the copy when the consumer's class asks
  Act o = hl_operand(ex, w, x, rows, C, nb, have_max);
  if (o.p != x.p) demote_lo(ex, cls, o, rows, C);
  return o;
}
// split-operand mode: q / o fp32, K [B][Nk][ldk] and V^T [B][H*64][vt_ld] in HL16 (attn_d64_hl_kernel)
void attention_hl(Exec& ex, const Act& q, const void* kh, int ldk, const void* vth, int vt_ld, const Act& o, int B, int H, int Nq, int Nk, int demote_cls = 0) {
  if (ex.dry) return;
  AttnParams p{};
  p.demote = (ex.demote & demote_cls) ? 1 : 0;
  p.Q = q.p; p.ldq = q.ld; p.K = kh; p.ldk = ldk; p.Vt = vth; p.vt_ld = vt_ld; p.O = o.p; p.ldo = o.ld;
  p.dt = DT_HL; p.B = B; p.H = H; p.Nq = Nq; p.Nk = Nk; p.scale = 0.125f; p.mask = nullptr; p.ldmask = 0;
  p.o_dt = o.dt == DT_HL ? DT_HL : o.dt == DT_F16 ? DT_F16 : DT_F32;
  p.q_dt = q.dt == DT_HL ? DT_HL : DT_F32;
  if (ex.prof) ex.prof->begin(Profiler::ATTENTION, 4.0 * B * H * (double)Nq * Nk * 64, ex.s, Nq, Nk, B * H, 0, demote_cls);
  if (!launch_attention_d64_hl(p, ex.s)) throw Error("split-operand attention: unsupported shape / alignment (Nq=" + std::to_string(Nq) + " Nk=" + std::to_string(Nk) + ")");
  {
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) throw Error(std::string("split-operand attention launch failed (") + hipGetErrorString(le) + ")");
  }
  if (ex.prof) ex.prof->end(ex.s);
}
}  // namespace

void alloc_ln_operands(Exec& ex, const StPlan& pl, size_t M, int C, const Act& ln, LnOperands& o) {
  o.M = M; o.C = C; o.ln = ln; o.have_sh = false;
  if (reads_f16(pl.geglu) || pl.qkv == LF_F16 || pl.q2 == LF_F16) o.ln16 = ex.alloc(M, C, DT_F16);
  // (hi | lo) GEGLU forms: the LayerNorm launch writes [a | a 2^-8] or [a_hi | a_lo 2^8] along a doubled K
  if (pl.geglu == LF_F16_WHILO || pl.geglu == LF_F16_AHILO) o.ln16x2 = ex.alloc(M, 2 * C, DT_F16);
  if (pl.qkv_sh || pl.q2_sh || pl.geglu_sh) { o.sh16 = ex.alloc(M, C, DT_F16); o.shst = (float*)ex.act->alloc(M * (size_t)((C + 63) / 64) * 2 * sizeof(float)); }
  if (pl.geglu_sh && pl.geglu == LF_F16_AHILO) o.sh16g = ex.alloc(M, 2 * C, DT_F16);
  if ((pl.qkv_sh && pl.qkv == LF_X2) || (pl.q2_sh && pl.q2 == LF_X2) || (pl.geglu_sh && pl.geglu == LF_X2)) o.shhl = ex.alloc(M, C, DT_HL);
}
void want_ln_shadow(LnOperands& o, Epi& e, bool sh, LinForm f, const NormW& n) {
  o.have_sh = false;
  if (!sh || o.C % 64 != 0) return;
  e.shadow = o.sh16.p; e.shadow_ld = o.sh16.ld; e.shadow_gamma = n.gamma; e.stat_out = o.shst; e.shadow_done = &o.have_sh;
  if (f == LF_F16_AHILO) { e.shadow = o.sh16g.p; e.shadow_ld = o.sh16g.ld; e.shadow_lo_scale = kHiLoScale; }      // (hi | lo) halves: the consumer's K is doubled
  if (f == LF_X2) { e.shadow = o.shhl.p; e.shadow_ld = o.shhl.ld; e.shadow_lo_scale = -1.f; }      // HL16 rows
}
LnIn ln_input(Exec& ex, LnOperands& o, const Lin& plain, const Lin& sh, LinForm f, const NormW& n, const Act& t, int cls) {
  const bool from_sh = o.have_sh;
  o.have_sh = false;
  if (from_sh) return LnIn{&sh, f == LF_X2 ? Act(o.shhl.p, 2 * o.shhl.ld, DT_F16) : f == LF_F16_AHILO ? o.sh16g : o.sh16, o.shst};
  if (f == LF_F16_WHILO || f == LF_F16_AHILO) {
    run_layernorm(ex, n, t, (int)o.M, o.ln16x2, f == LF_F16_AHILO ? -kHiLoScale : 1.0f / kHiLoScale);
    return LnIn{&plain, o.ln16x2, nullptr};
  }
  run_layernorm(ex, n, t, (int)o.M, f == LF_F16 ? o.ln16 : o.ln);
  demote_lo(ex, cls, o.ln, o.M, o.C);
  return LnIn{&plain, f == LF_F16 ? o.ln16 : x2_operand(f, o.ln), nullptr};
}

static std::atomic<int> g_mix_classes{-1};     // A/B / debugging knob (sdxl_debug_set "mix_classes"): overrides the MixClass bits of SDXL_DTYPE_F32_SPLIT_MIX models built afterwards (-1 = the mode's own)
void unet_set_mix_classes(int v) { g_mix_classes = v; }
static std::atomic<int> g_hl_demote{0};
void unet_set_hl_demote(int mask) { g_hl_demote = mask; }
static std::atomic<int> g_xattn_long{1};
void unet_set_xattn_long(int v) { g_xattn_long = v; }
int unet_hl_demote() { return g_hl_demote.load(); }

// the exact-f16 flag (acc_scale[1]) of every packed matrix of a demoted class reads 1 -- the kernel then leaves its w_lo MFMAs out --
// and its packed value otherwise; the packed values are read back once
void UNet::apply_demote_weights(hipStream_t s) {
  if (cdt_ != DT_HL) return;
  if (demote_flags_.empty()) {
    auto add = [&](const Lin& l, int cls) {
      if (!l.acc_scale) return;
      float v = 0.f;
      SDXL_HIP(hipMemcpy(&v, l.acc_scale + 1, sizeof(float), hipMemcpyDeviceToHost));
      demote_flags_.push_back({const_cast<float*>(l.acc_scale) + 1, v}); demote_flag_cls_.push_back(cls);
    };
    auto add_res = [&](const ResBlockW& r) { add(r.conv_in, DM_CONV_RES); add(r.conv_out, DM_CONV_RES); if (r.has_skip) add(r.skip, DM_CONV_SKIP); };
    auto add_st = [&](const STW& st) {
      add(st.proj_in, DM_CONV_PROJ); add(st.proj_out, DM_CONV_PROJ);
      for (const TBlockW& b : st.blocks) {
        add(b.qkv, DM_QKV); add(b.out1, DM_OUT); add(b.q2, DM_XATTN); add(b.kv2, DM_XATTN); add(b.out2, DM_OUT); add(b.geglu, DM_GEGLU); add(b.ff, DM_FF);
      }
    };
    auto add_block = [&](const BlockW& b) { add(b.conv, b.d.kind == BK_CONV ? DM_CONV_IO : DM_CONV_UPDOWN); add_res(b.res); add_st(b.st); };
    for (const BlockW& b : inp_) add_block(b);
    add_block(mid_res1_); add_res(mid_res2_.res);
    for (const BlockW& b : out_) add_block(b);
    add(conv_out_, DM_CONV_IO);
  }
  std::vector<float> vals(demote_flags_.size());
  for (size_t i = 0; i < demote_flags_.size(); ++i) {
    vals[i] = (demote_mask_ & demote_flag_cls_[i]) ? 1.0f : demote_flags_[i].second;
    SDXL_HIP(hipMemcpyAsync(demote_flags_[i].first, &vals[i], sizeof(float), hipMemcpyHostToDevice, s));
  }
  SDXL_HIP(hipStreamSynchronize(s));     // (vals is host memory of this frame)
}

UNet::UNet(const UNetCfg& cfg, int compute_dt, int stream_dt, int mix) : cfg_(cfg), cdt_(compute_dt), sdt_(stream_dt), mix_(compute_dt == DT_HL ? mix : 0) {
  SDXL_REQUIRE(cfg.n_head_channels == 64, "this engine's fused attention kernel is specialised for 64 channels per head");
  SDXL_REQUIRE(!((compute_dt == DT_F32 || compute_dt == DT_HL) && stream_dt != DT_F32), "f32 / split-operand compute implies an f32 residual stream");
  SDXL_REQUIRE(cfg.model_channels % 32 == 0, "GroupNorm(32) needs model_channels % 32 == 0");
  fuse_ln_ = compute_dt == DT_F16 && stream_dt == DT_F16;
  mix_mode_ = mix_ != 0;
}
UNet::UNet(const UNetCfg& cfg, int compute_dt, int stream_dt, WeightSource& src, hipStream_t st, int mix)
    : UNet(cfg, compute_dt, stream_dt, mix && g_mix_classes.load() >= 0 ? g_mix_classes.load() : mix) {
  mix_knob_ = compute_dt == DT_HL && mix && g_mix_classes.load() >= 0;
  build_weights(src, st);
}
size_t UNet::weight_layout_bytes(const UNetCfg& cfg, int compute_dt, int stream_dt, int mix) {
  UNet u(cfg, compute_dt, stream_dt, mix);
  const std::vector<ParamSpec> specs = unet_param_specs(cfg);
  return u.layout_weights(specs, u.plan_transformers(specs, nullptr));
}
UNet::UNet(const ControlCfg& cfg, int compute_dt, int stream_dt, WeightSource& src, hipStream_t st) : UNet(cfg.unet, compute_dt, stream_dt, 0) {
  control_ = true;
  ccfg_ = cfg;
  build_weights(src, st);
}
UNet::~UNet() {
  if (graph_) (void)hipGraphExecDestroy(graph_);
  if (ev_fork_) (void)hipEventDestroy(ev_fork_);
  if (ev_join_) (void)hipEventDestroy(ev_join_);
  if (s2_) (void)hipStreamDestroy(s2_);
}

// the plans of the spatial transformers in build order (input blocks, middle block, output blocks) for the classes in force; f16_names: + the weights
// those plans pack as f16 values
std::vector<StPlan> UNet::plan_transformers(const std::vector<ParamSpec>& specs, std::vector<std::string>* f16_names) const {
  std::vector<BlockDesc> inp, out; BlockDesc mid;
  unet_block_plan(cfg_, inp, mid, out);
  std::vector<StPlan> plans;
  auto add = [&](const std::string& p, const BlockDesc& d, bool has_st) {
    if (!has_st) return;
    plans.push_back(plan_transformer(mix_, cdt_, specs, p + ".transformer"));
    for (int j = 0; f16_names && j < d.depth; ++j) f16_valued_weights(plans.back(), p + ".transformer.blocks." + std::to_string(j), *f16_names);
  };
  auto has_st = [](const BlockDesc& d) { return d.kind == BK_REST || d.kind == BK_RESTU; };
  for (size_t i = 0; i < inp.size(); ++i) add("input_blocks." + std::to_string(i), inp[i], has_st(inp[i]));
  add("middle_block", mid, true);
  for (size_t i = 0; !control_ && i < out.size(); ++i) add("output_blocks." + std::to_string(i), out[i], has_st(out[i]));
  return plans;
}
// the arena bytes load_weights allocates: the loader over a dry arena and an empty source (no device call)
size_t UNet::layout_weights(const std::vector<ParamSpec>& specs, const std::vector<StPlan>& plans) {
  DeviceArena dry; dry.dry = true;
  NullSource none;
  WeightBuilder wb(specs, none, dry, cdt_, nullptr);
  load_weights(wb, plans);
  return dry.peak;
}
void UNet::build_weights(WeightSource& src, hipStream_t st) {
  const std::vector<ParamSpec> specs = control_ ? controlnet_param_specs(ccfg_) : unet_param_specs(cfg_);
  std::vector<std::string> f16_names;
  std::vector<StPlan> plans = plan_transformers(specs, &f16_names);
  WeightBuilder wb(specs, src, warena_, cdt_, st);
  // A form that packs a parameter's values as f16 (StPlan) must get f16 values (the reference's records are, src/bin/sample/main.rs:37): on other
  // parameters it would round the weights as well and leave the mode's error bound (0.029 against 0.0212).  Checked here on exactly those
  // tensors; a model that does not qualify falls back to F32_SPLIT_MIX's classes (capi_internal.h mix_of) -- plain F32_SPLIT for a mode without f16-OPERAND classes,
  // SDXL_DTYPE_F32_SPLIT_F16W -- and mix_classes() tells.
  // Not applied to the A/B knob "mix_classes" (the frontier tools run those maps on fp32 weights on purpose) nor on replicas built from an empty
  // source (they receive rank 0's arena: the caller compares rank 0's mix_classes() with the mode before the broadcast, bench.py does).
  if (!mix_knob_ && !wb.all_f16_exact(f16_names)) {
    mix_ = (mix_ & (MIX_ATTN_F16 | MIX_GEGLU_F16)) ? (MIX_ATTN_F16 | MIX_GEGLU_F16 | MIX_GEGLU_HILO) : 0;
    f16_names.clear();
    plans = plan_transformers(specs, &f16_names);
    SDXL_REQUIRE(f16_names.empty(), "the fallback classes pack no parameter as f16 values");
  }
  // the plans are final: size the arena by a layout pass of the loader, then run it for real
  warena_.reserve(layout_weights(specs, plans));
  load_weights(wb, plans);
  SDXL_HIP(hipStreamSynchronize(st));
}
void UNet::load_weights(WeightBuilder& wb, const std::vector<StPlan>& plans) {
  std::vector<BlockDesc> inp, out; BlockDesc mid;
  unet_block_plan(cfg_, inp, mid, out);
  inp_.clear(); out_.clear(); st_list_.clear();
  attn16_ = cdt_ == DT_F16;
  for (const StPlan& pl : plans) attn16_ = attn16_ || pl.attn_f16;
  const int gv = gemv_weight_dt(cdt_);     // the M <= 8 GEMV weights of a split-operand model are packed fp32
  lin1_t_ = wb.linear("lin1_time_embed", false, gv);
  lin2_t_ = wb.linear("lin2_time_embed", false, gv);
  lin1_l_ = wb.linear("lin1_label_embed", false, gv);
  lin2_l_ = wb.linear("lin2_label_embed", false, gv);
  std::vector<std::string> emb_names;
  int emb_off = 0;
  size_t sti = 0;
  auto load_block = [&](const std::string& p, const BlockDesc& d) {
    BlockW b; b.d = d;
    switch (d.kind) {
      case BK_CONV: case BK_DOWN: b.conv = wb.conv(p); break;
      case BK_RES: b.res = load_res(wb, p, d.c_in, d.c_out, emb_names, emb_off); break;
      default:
        b.res = load_res(wb, p + ".res", d.c_in, d.c_out, emb_names, emb_off);
        if (d.kind == BK_REST || d.kind == BK_RESTU) b.st = load_st(wb, p + ".transformer", d.c_out, d.n_head, d.depth, fuse_ln_, plans[sti++]);
        if (d.kind == BK_RESTU || d.kind == BK_RESU) b.conv = wb.conv(p + ".upsample.conv", fuse_ln_);      // f16 engine: + the folded phase matrices (Lin::w_fold)
    }
    return b;
  };
  for (size_t i = 0; i < inp.size(); ++i) inp_.push_back(load_block("input_blocks." + std::to_string(i), inp[i]));
  mid_res1_.d = mid;
  mid_res1_.res = load_res(wb, "middle_block.res1", mid.c_in, mid.c_out, emb_names, emb_off);
  mid_res1_.st = load_st(wb, "middle_block.transformer", mid.c_out, mid.n_head, mid.depth, fuse_ln_, plans[sti++]);
  mid_res2_.d = mid;
  mid_res2_.res = load_res(wb, "middle_block.res2", mid.c_in, mid.c_out, emb_names, emb_off);
  if (!control_) {
    for (size_t i = 0; i < out.size(); ++i) out_.push_back(load_block("output_blocks." + std::to_string(i), out[i]));
    norm_out_ = wb.norm("norm_out");
    conv_out_ = wb.conv("conv_out");
  } else {      // hint embedder, one 1x1 convolution per residual tensor
    for (int k = 0; k < 8; ++k) hint_conv_[k] = wb.conv("input_hint_block." + std::to_string(k));
    zero_.clear();
    for (size_t i = 0; i < inp.size(); ++i) zero_.push_back(wb.conv("zero_convs." + std::to_string(i)));
    mid_out_ = wb.conv("middle_block_out");
  }
  embcat_ = wb.fused_linear(emb_names, gv);
  emb_total_ = emb_off;
  // execution order of the spatial transformers (for the K/V caches)
  for (BlockW& b : inp_) if (!b.st.blocks.empty()) st_list_.push_back(&b.st);
  st_list_.push_back(&mid_res1_.st);
  for (BlockW& b : out_) if (!b.st.blocks.empty()) st_list_.push_back(&b.st);      // (none in control mode)
}

// ------------------------------------------------------------------------------------------ conditioning
void UNet::set_context(const float* context, int n_ctx, const float* label, int B, hipStream_t s) {
  SDXL_REQUIRE(B >= 1 && B <= 8, "batch must be in 1..8");
  const int vt_ld = (int)round_up(n_ctx, 64);
  // operand-order copies for the fused cross-attention epilogue (f16 engines; the split-operand engine when that class runs on f16: MIX_XATTN_F16)
  // (MIX_XATTN_SPLIT: TWO images -- the hi and the lo halves of the fp32-class projection -- for the split-precision form of that epilogue)
  bool pack_xs = false, pack_xa = false;
  for (const STW* st : st_list_) { pack_xs = pack_xs || st->plan.xattn == XA_SPLIT; pack_xa = pack_xa || st->plan.xattn != XA_LAUNCH; }
  // more than 96 keys (a prompt of two to four 77-token chunks): the blocked image, where the weights-in-registers form of the fused launch will take
  // a transformer's width (igemm_xattn_ok -- the predicate spatial_transformer and the selection ask; rows per entry are not known here: one 64-row
  // entry stands in, the forward asks again with its own) and the knob "xattn_long" allows it; the split-precision form keeps its 96 keys
  bool long_ok = false;
  if (n_ctx > 96 && g_xattn_long.load()) {
    const SelectKnobs knobs = igemm_launch_knobs();
    for (const STW* st : st_list_)
      if (!st->blocks.empty())
        long_ok = long_ok || igemm_xattn_ok(DT_F16, DT_F16, 64, st->C, st->C, 64, n_ctx, knobs, st->blocks[0].q2.wf || st->blocks[0].q2_sh.wf);
  }
  pack_xs = pack_xs && n_ctx <= 96; pack_xa = pack_xa && (n_ctx <= 96 || long_ok);
  const int kvdt = attn_dt();                           // dtype of the K / V^T caches (fp32 in the split-operand mode)
  const int emb = 4 * cfg_.model_channels;
  {   // precision-frontier instrument: the demoted classes take effect from here (weights now, activations in every forward after)
    const int dm = cdt_ == DT_HL ? unet_hl_demote() : 0;
    if (dm != demote_mask_ || (dm && demote_flags_.empty())) { demote_mask_ = dm; apply_demote_weights(s); }
  }
  if (B != ctx_B_ || n_ctx != n_ctx_ || pack_xa != ctx_xa_) {
    // (re)allocate the caches; captured graphs hold these addresses
    if (graph_) { (void)hipGraphExecDestroy(graph_); graph_ = nullptr; plan_runs_ = 0; }
    // the recorded warming schedule holds raw pointers into ctx_arena_ (the packed context of the fused cross-attention
    // projections is a warm target): a re-laid-out / reallocated arena invalidates them -> record again on the next eager forward
    warm_ = WarmSeq();
    plan_runs_ = 0;
    size_t bytes = 1 << 16;
    for (const STW* st : st_list_)
      bytes += st->blocks.size() * (round_up((size_t)B * n_ctx * st->C * dt_size(kvdt), 256) +
                                    round_up((size_t)B * st->C * vt_ld * dt_size(kvdt), 256) +
                                    (pack_xa ? round_up(xattn_pack_bytes(B, st->C, n_ctx), 256) : 0) + (pack_xs ? round_up(xattn_pack_bytes(B, st->C, n_ctx), 256) : 0) + 768);
    bytes += 3 * round_up((size_t)B * emb * sizeof(float), 256);
    if (cdt_ == DT_HL) bytes += round_up((size_t)B * n_ctx * cfg_.context_dim * 4, 256) + 256;   // HL16 copy of the context
    if (cdt_ == DT_HL) {   // fp32 scratch of one block's K / V^T projection: the caches themselves are HL16 (what the attention kernel reads)
      size_t mx = 0;
      for (const STW* st : st_list_) mx = std::max(mx, round_up((size_t)B * n_ctx * st->C * 4, 256) + round_up((size_t)B * st->C * vt_ld * 4, 256));
      bytes += (pack_xs ? 2 * mx + 1024 : pack_xa ? mx + mx / 2 + 512 : mx) + 512;     // (+ f16 copies of both -- hi and lo with MIX_XATTN_SPLIT -- when the fused cross-attention reads them packed)
    }
    ctx_arena_.reserve(bytes);
    ctx_arena_.off = 0;
    SDXL_HIP(hipMemsetAsync(ctx_arena_.base, 0, bytes, s));   // V^T key padding must be zero
    kv_.clear();
    for (const STW* st : st_list_) {
      std::vector<KV> v;
      for (size_t j = 0; j < st->blocks.size(); ++j) {
        KV kv;
        kv.k = ctx_arena_.alloc((size_t)B * n_ctx * st->C * dt_size(kvdt));
        kv.vt = ctx_arena_.alloc((size_t)B * st->C * vt_ld * dt_size(kvdt));
        if (pack_xa) kv.xa = ctx_arena_.alloc(xattn_pack_bytes(B, st->C, n_ctx));
        if (pack_xs) kv.xa_lo = ctx_arena_.alloc(xattn_pack_bytes(B, st->C, n_ctx));
        v.push_back(kv);
      }
      kv_.push_back(v);
    }
    label_emb_ = (float*)ctx_arena_.alloc((size_t)B * emb * sizeof(float));
    ctx_B_ = B; n_ctx_ = n_ctx; vt_ld_ctx_ = vt_ld; ctx_xa_ = pack_xa;
  }
  Exec ex; ex.s = s; ex.cdt = cdt_; ex.sdt = sdt_; ex.act = &ctx_arena_; ex.demote = demote_mask_;
  const size_t m0 = ctx_arena_.mark();
  Act ctx((void*)context, cfg_.context_dim, DT_F32);
  if (cdt_ == DT_HL && !st_list_.empty() && !st_list_[0]->blocks.empty()) {    // one HL16 copy of the context for all 70 projections
    ctx = hl_operand(ex, st_list_[0]->blocks[0].kv2, ctx, (size_t)B * n_ctx, cfg_.context_dim, B);
    demote_lo(ex, DM_XATTN, ctx, (size_t)B * n_ctx, cfg_.context_dim);
  }
  for (size_t si = 0; si < st_list_.size(); ++si) {
    const STW* st = st_list_[si];
    for (size_t j = 0; j < st->blocks.size(); ++j) {
      if (cdt_ == DT_HL) {
        const size_t ms = ctx_arena_.mark();
        void* k32 = ctx_arena_.alloc((size_t)B * n_ctx * st->C * 4);
        void* vt32 = ctx_arena_.alloc((size_t)B * st->C * vt_ld * 4);
        launch_fill_zero(vt32, (size_t)B * st->C * vt_ld * 4, s);                     // V^T key padding must be zero
        Epi e; e.n_split = st->C; e.Ct = vt32; e.ct_rows = st->C; e.ct_ld = vt_ld; e.rpb = n_ctx; e.cls = DM_XATTN;
        run_linear(ex, st->blocks[j].kv2, ctx, B * n_ctx, Act(k32, st->C, DT_F32), e);
        launch_f32_to_hl(k32, st->C, kv_[si][j].k, st->C, (size_t)B * n_ctx, st->C, s);
        launch_f32_to_hl(vt32, vt_ld, kv_[si][j].vt, vt_ld, (size_t)B * st->C, vt_ld, s);
        demote_lo(ex, DM_XATTN, Act(kv_[si][j].k, st->C, DT_HL), (size_t)B * n_ctx, st->C);
        demote_lo(ex, DM_XATTN, Act(kv_[si][j].vt, vt_ld, DT_HL), (size_t)B * st->C, vt_ld);
        if (kv_[si][j].xa_lo) {  // MIX_XATTN_SPLIT: hi = f16(x), lo = f16(x - hi) of the fp32-class projection, each in the operand order the fused launch reads
          void* kh = ctx_arena_.alloc((size_t)B * n_ctx * st->C * 2); void* kl = ctx_arena_.alloc((size_t)B * n_ctx * st->C * 2);
          void* vh = ctx_arena_.alloc((size_t)B * st->C * vt_ld * 2); void* vl = ctx_arena_.alloc((size_t)B * st->C * vt_ld * 2);
          launch_f32_to_f16_pair((const float*)k32, st->C, kh, kl, st->C, (size_t)B * n_ctx, st->C, s);
          launch_f32_to_f16_pair((const float*)vt32, vt_ld, vh, vl, vt_ld, (size_t)B * st->C, vt_ld, s);
          launch_xattn_pack(kh, vh, kv_[si][j].xa, B, st->C, n_ctx, vt_ld, s);
          launch_xattn_pack(kl, vl, kv_[si][j].xa_lo, B, st->C, n_ctx, vt_ld, s);
        } else
        if (kv_[si][j].xa) {     // MIX_XATTN_F16: the fp32-class projection rounded once to f16, in the operand order the fused launch reads
          void* k16 = ctx_arena_.alloc((size_t)B * n_ctx * st->C * 2);
          void* vt16 = ctx_arena_.alloc((size_t)B * st->C * vt_ld * 2);
          launch_copy_rows(k32, DT_F32, st->C, k16, DT_F16, st->C, B * n_ctx, st->C, s);
          launch_copy_rows(vt32, DT_F32, vt_ld, vt16, DT_F16, vt_ld, B * st->C, vt_ld, s);
          launch_xattn_pack(k16, vt16, kv_[si][j].xa, B, st->C, n_ctx, vt_ld, s);
        }
        ctx_arena_.reset(ms);
        continue;
      }
      Epi e; e.n_split = st->C; e.Ct = kv_[si][j].vt; e.ct_rows = st->C; e.ct_ld = vt_ld; e.rpb = n_ctx; e.cls = DM_XATTN;
      run_linear(ex, st->blocks[j].kv2, ctx, B * n_ctx, Act(kv_[si][j].k, st->C, kvdt), e);
      if (kv_[si][j].xa) launch_xattn_pack(kv_[si][j].k, kv_[si][j].vt, kv_[si][j].xa, B, st->C, n_ctx, vt_ld, s);
    }
  }
  ctx_arena_.reset(m0);
  // label embedding MLP (unet/mod.rs:464-466); scratch after the caches
  label_valid_ = label != nullptr;
  if (!label) return;      // (run_block: its caller hands in t_emb + l_emb; forward refuses to run on what is left in label_emb_)
  const size_t m = ctx_arena_.mark();
  float* l1 = (float*)ctx_arena_.alloc((size_t)B * emb * sizeof(float));
  gemv(ex, lin1_l_, label, cfg_.adm_in_channels, l1, emb, B, false, true);
  gemv(ex, lin2_l_, l1, emb, label_emb_, emb, B, false, false);
  ctx_arena_.reset(m);
}

// ------------------------------------------------------------------------------------------ blocks
const float* UNet::res_block(Exec& ex, const ResBlockW& w, const Act& x, int B, int H, int W, const Act& out, float* out_gn_part) {
  // ResBlock::forward unet/mod.rs:1082-1106.  GroupNorm statistics ride on the producing convolutions where their kernel can
  // leave them (256-row tiles: the 64^2 and 32^2 levels): the second norm never runs a statistics pass there, and the caller
  // gets the statistics of `out` (returned pointer, null if not produced) for the SpatialTransformer norm that follows.
  const size_t mk = ex.act->mark();
  const size_t M = (size_t)B * H * W;
  const int HW = H * W;
  const ConvGeom g3{B, H, W, H, W, 3, 1, 1, 0}, g1{B, H, W, H, W, 1, 1, 0, 0};
  const bool tiles256 = gn_from_producer_ && HW % 256 == 0;
  Act gn1 = ex.alloc(M, w.cin, ex.cdt);
  // split-operand engines: the 1x1 skip convolution reads x as an HL16 copy scaled per entry by max|x| -- the statistics pass of norm_in reads all
  // of x anyway and leaves the maxima, so that copy needs no absmax pass of its own (11 launches of a step)
  float* skip_max = nullptr;
  if (w.has_skip && ex.cdt == DT_HL && x.dt == DT_F32 && w.skip.dt != DT_F32 && !x.gn_part && M % (size_t)B == 0)
    skip_max = (float*)ex.act->alloc(hl_scale_floats(B) * sizeof(float));
  run_groupnorm(ex, w.norm_in, x, B, HW, gn1, true, 32, skip_max);
  demote_lo(ex, DM_CONV_RES, gn1, M, w.cin);
  Act h = ex.alloc(M, w.cout, ex.cdt == DT_HL ? ex.sdt : ex.cdt);     // (read by a GroupNorm only: fp32 in the split-operand mode)
  Epi e1; e1.ebias = ex.ebias + w.emb_off; e1.ebias_ld = emb_total_; e1.cls = DM_CONV_RES;
  if (tiles256) e1.gn_part = (float*)ex.act->alloc(M / 256 * (size_t)w.cout * 2 * sizeof(float));
  if (run_conv(ex, w.conv_in, gn1, w.cin, g3, h, e1)) { h.gn_part = e1.gn_part; h.gn_rt = HW / 256; }
  Act gn2 = ex.alloc(M, w.cout, ex.cdt);
  run_groupnorm(ex, w.norm_out, h, B, HW, gn2, true);
  demote_lo(ex, DM_CONV_RES, gn2, M, w.cout);
  Epi e2; e2.cls = DM_CONV_RES;
  if (w.has_skip) { Epi es; es.cls = DM_CONV_SKIP; run_conv(ex, w.skip, hl_op(ex, w.skip, x, M, w.cin, DM_CONV_SKIP, B, skip_max), w.cin, g1, out, es); e2.R = out; }
  else e2.R = x;
  if (tiles256) e2.gn_part = out_gn_part;
  const bool produced = run_conv(ex, w.conv_out, gn2, w.cout, g3, out, e2);
  ex.act->reset(mk);
  return produced ? out_gn_part : nullptr;
}

void UNet::spatial_transformer(Exec& ex, const STW& w, int si, const Act& x, int B, int H, int W) {
  // SpatialTransformer::forward unet/mod.rs:820-845, TransformerBlock::forward :885-891 -- in place on x
  const size_t mk = ex.act->mark();
  const int HW = H * W, C = w.C;
  const size_t M = (size_t)B * HW;
  SDXL_REQUIRE(C == w.heads * 64, "head dim must be 64");
  const int npad = (int)round_up(HW, 64);
  // cross-attention caches of this run's batch entries (dry runs carry null caches)
  const int adt = attn_dt();      // q / k / V^T / attention output: the compute dtype, fp32 in the split-operand mode
  auto kv_k = [&](int s_, size_t j) { char* k = (char*)kv_[s_][j].k; return (void*)(k ? k + (size_t)ex.b0 * n_ctx_ * C * dt_size(adt) : k); };
  auto kv_xa = [&](int s_, size_t j) { char* v = (char*)kv_[s_][j].xa; return (const void*)(v ? v + xattn_pack_bytes(ex.b0, C, n_ctx_) : v); };
  auto kv_xa_lo = [&](int s_, size_t j) { char* v = (char*)kv_[s_][j].xa_lo; return (const void*)(v ? v + xattn_pack_bytes(ex.b0, C, n_ctx_) : v); };
  auto kv_vt = [&](int s_, size_t j) { char* v = (char*)kv_[s_][j].vt; return (const void*)(v ? v + (size_t)ex.b0 * C * vt_ld_ctx_ * dt_size(adt) : v); };
  Act gn = ex.alloc(M, C, ex.cdt);
  run_groupnorm(ex, w.norm, x, B, HW, gn, false);
  demote_lo(ex, DM_CONV_PROJ, gn, M, C);
  Act t = ex.alloc(M, C, ex.sdt);
  // cross-attention fused into the query projection (f16 operands; igemm_xattn_ok: up to 96 context tokens in every form, up to 384 where the
  // weights-in-registers form takes the launch and set_context packed the blocked image)
  const SelectKnobs xknobs = igemm_launch_knobs();
  const bool xa_img = n_ctx_ <= 96 || ctx_xa_;
  const bool xattn = plan_xattn_ && xa_img && igemm_xattn_ok(fuse_ln_ ? ex.sdt : ex.cdt, ex.cdt, (int)M, C, C, HW, n_ctx_, xknobs, !w.blocks.empty() && w.blocks[0].q2.wf);
  // folded LayerNorms: two ping-pong [M][C/64][2] partial-sum buffers -- each is written by one GEMM and read by the next
  float* stbuf[2] = {nullptr, nullptr};
  if (fuse_ln_) for (int i = 0; i < 2; ++i) stbuf[i] = (float*)ex.act->alloc(M * (size_t)(C / 64) * 2 * sizeof(float));
  int stp = 0;
  { Epi ep; ep.stat_out = w.blocks.empty() ? nullptr : stbuf[stp]; ep.rpb = HW; ep.cls = DM_CONV_PROJ; run_linear(ex, w.proj_in, gn, (int)M, t, ep); }   // (rpb: kernel selection looks at ONE entry's rows)
  Act ln = ex.alloc(M, C, ex.cdt);
  // (split-operand mode: the projections write q | k and V^T as HL16 -- 4 bytes per element like fp32 -- what attention_hl reads)
  // (HL16 pieces are 8 keys wide: token counts that are not multiples of 8 -- tiny test nets -- go through fp32 + a conversion)
  const bool hl_direct = ex.cdt == DT_HL && HW % 8 == 0 && (2 * C) % 128 == 0;
  const int qdt = hl_direct ? DT_HL : adt;
  Act qk = ex.alloc(M, 2 * C, qdt);
  void* vt = ex.act->alloc((size_t)B * C * npad * dt_size(adt));
  Act ao = ex.alloc(M, C, ex.cdt);
  Act q = ex.alloc(M, C, qdt);
  Act gg = ex.alloc(M, 4 * C, ex.cdt);
  // (split-operand mode: attention_hl writes the out-projection's HL16 operand `ao` itself)
  if (npad != HW && !ex.dry) launch_fill_zero(vt, (size_t)B * C * npad * dt_size(adt), ex.s);
  // split-operand mode: the attention kernel takes K and V^T in HL16 (same bytes as fp32); q and the output stay fp32
  const bool hl_attn = ex.cdt == DT_HL;
  // forms of the projections (plan_transformer; mixed modes SDXL_DTYPE_F32_SPLIT_MIX*: classes chosen on the measured precision frontier,
  // profiles/r05_precision_frontier.json):
  //   * self-attention on the f16 flash kernels: the QKV projection writes q | k and V^T as f16, the attention output is handed to the
  //     out-projection as HL16 with zero lo halves (an f16 value is its own hi half) -- or as it is to an f16 one;
  //   * f16 projections read an f16 LayerNorm output; an f16 GEGLU projection's output leaves the epilogue as HL16 (fp32-class), so FF-out's
  //     operand is not rounded a second time (an f16 FF-out reads it as f16).
  const StPlan& pl = w.plan;
  Act ao2_16;      // operand of an f16 cross-attention out-projection: the split-operand attention rounds its fp32 result once, in its own store (AttnParams::o_dt)
  if (pl.out2 == LF_F16) ao2_16 = ex.alloc(M, C, DT_F16);
  const Act ao2 = pl.out2 == LF_F16 ? ao2_16 : ao;      // what the cross-attention writes: the out-projection's operand
  Act qk16, ao16; void* vt16 = nullptr;
  if (pl.attn_f16) {
    qk16 = ex.alloc(M, 2 * C, DT_F16); ao16 = ex.alloc(M, C, DT_F16);
    vt16 = ex.act->alloc((size_t)B * C * npad * 2);
    if (npad != HW && !ex.dry) launch_fill_zero(vt16, (size_t)B * C * npad * 2, ex.s);
  }
  // the LayerNorm outputs of the forms and the shadow the producers leave (LnOperands)
  LnOperands lo;
  alloc_ln_operands(ex, pl, M, C, ln, lo);
  // the knob's f16 fused cross-attention on shapes its launch does not take: f16 q, widened for the split-operand attention
  const bool q2_widen = hl_attn && pl.xattn == XA_F16;
  Act q32;     // f16 query projection: fp32 q for the split-operand attention (the projection's fp32 accumulators, never rounded to f16)
  if (pl.q2 == LF_F16 && !q2_widen) q32 = ex.alloc(M, C, DT_F32);
  // cross-attention inside the query projection's epilogue (the context images of set_context): q never reaches memory, no attention launch
  const bool xa_fused = pl.xattn != XA_LAUNCH && plan_xattn_ && !w.blocks.empty() && (pl.xattn == XA_SPLIT ? kv_[si][0].xa_lo : kv_[si][0].xa) &&
                        igemm_xattn_ok(DT_F16, ao2.dt, (int)M, C, pl.q2 == LF_X2 ? 2 * C : C, HW, n_ctx_, xknobs,
                                       pl.xattn == XA_F16 && w.blocks[0].q2.wf && (!pl.q2_sh || w.blocks[0].q2_sh.wf));      // (ln_input picks either weight)
  auto want_shadow = [&](Epi& e, bool sh, LinForm f, const NormW& n) { want_ln_shadow(lo, e, sh, f, n); };
  auto ln_in = [&](const Lin& plain, const Lin& sh, LinForm f, const NormW& n, int cls) { return ln_input(ex, lo, plain, sh, f, n, t, cls); };
  const auto x2op = x2_operand;
  Act gg16;
  if ((reads_f16(pl.geglu) && M < kGegluDirectRows) || pl.ff == LF_F16) gg16 = ex.alloc(M, 4 * C, DT_F16);     // (an f16 FF-out reads the GEGLU output as f16, whichever kernel wrote it)
  void* kh = hl_attn && !hl_direct ? ex.act->alloc(M * (size_t)C * 4) : nullptr;
  void* vth = hl_attn && !hl_direct ? ex.act->alloc((size_t)B * C * npad * 4) : nullptr;
  if (fuse_ln_) {
    // LayerNorms folded into the consuming GEMMs: every producer of the residual stream t also accumulates the row
    // (sum, sum^2) its consumer needs, so no LayerNorm kernel runs and t is read by the projections directly
    SDXL_REQUIRE(w.blocks.empty() || w.blocks[0].qkv.cs, "transformer weights were not LayerNorm-folded");
    for (size_t j = 0; j < w.blocks.size(); ++j) {
      const TBlockW& b = w.blocks[j];
      Epi eq; eq.n_split = 2 * C; eq.Ct = vt; eq.ct_rows = C; eq.ct_ld = npad; eq.rpb = HW; eq.ln_stat = stbuf[stp]; eq.cls = DM_QKV;
      run_linear(ex, b.qkv, t, (int)M, qk, eq);
      attention(ex, qk, qk.cols(C), vt, npad, ao, B, w.heads, HW, HW);
      stp ^= 1;
      Epi e1; e1.R = t; e1.stat_out = stbuf[stp]; e1.rpb = HW; e1.cls = DM_OUT;
      run_linear(ex, b.out1, ao, (int)M, t, e1);
      Epi e2q; e2q.ln_stat = stbuf[stp]; e2q.rpb = HW; e2q.cls = DM_XATTN;
      if (xattn) {   // the projection's waves run the 77-key attention on their own q tiles: no q round trip, no launch
        e2q.xa_k = kv_xa(si, j); e2q.xa_nctx = n_ctx_; e2q.xa_scale = 0.125f;
        run_linear(ex, b.q2, t, (int)M, ao, e2q);
      } else {
        run_linear(ex, b.q2, t, (int)M, q, e2q);
        attention(ex, q, Act(kv_k(si, j), C, ex.cdt), kv_vt(si, j), vt_ld_ctx_, ao, B, w.heads, HW, n_ctx_);
      }
      stp ^= 1;
      Epi e2; e2.R = t; e2.stat_out = stbuf[stp]; e2.rpb = HW; e2.cls = DM_OUT;
      run_linear(ex, b.out2, ao, (int)M, t, e2);
      Epi eg; eg.act = 1; eg.ln_stat = stbuf[stp]; eg.rpb = HW; eg.cls = DM_GEGLU;
      run_linear(ex, b.geglu, t, (int)M, gg, eg);
      stp ^= 1;
      Epi ef; ef.R = t; ef.stat_out = j + 1 < w.blocks.size() ? stbuf[stp] : nullptr; ef.rpb = HW; ef.cls = DM_FF;
      run_linear(ex, b.ff, gg, (int)M, t, ef);
    }
  } else
  for (size_t j = 0; j < w.blocks.size(); ++j) {
    const TBlockW& b = w.blocks[j];
    const LnIn iq = ln_in(b.qkv, b.qkv_sh, pl.qkv, b.n1, DM_QKV);
    Epi eq; eq.n_split = 2 * C; eq.Ct = pl.attn_f16 ? vt16 : vt; eq.ct_rows = C; eq.ct_ld = npad; eq.rpb = HW; eq.cls = DM_QKV; eq.ln_stat = iq.stat;
    run_linear(ex, *iq.w, iq.a, (int)M, pl.attn_f16 ? qk16 : qk, eq);
    if (pl.attn_f16) {
      attention(ex, qk16, qk16.cols(C), vt16, npad, ao16, B, w.heads, HW, HW);
      if (!ex.dry && pl.out1 != LF_F16) launch_f16_to_hl(ao16.p, ao16.ld, ao.p, ao.ld, M, C, ex.s);
    }
    else if (hl_attn && hl_direct) {     // q | k and V^T are HL16; the attention writes the out-projection's operand
      demote_lo(ex, DM_ATTN, qk, M, 2 * C);
      demote_lo(ex, DM_ATTN, Act(vt, npad, DT_HL), (size_t)B * C, npad);
      attention_hl(ex, qk, qk.cols(C).p, qk.ld, vt, npad, ao, B, w.heads, HW, HW, DM_ATTN);
    }
    else if (hl_attn) {
      if (!ex.dry) {
        launch_f32_to_hl(qk.cols(C).p, qk.ld, kh, C, M, C, ex.s);
        launch_f32_to_hl(vt, npad, vth, npad, (size_t)B * C, npad, ex.s);
      }
      attention_hl(ex, qk, kh, C, vth, npad, ao, B, w.heads, HW, HW);
    }
    else attention(ex, qk, qk.cols(C), vt, npad, ao, B, w.heads, HW, HW);
    Epi er; er.R = t; er.rpb = HW; er.cls = DM_OUT;
    demote_lo(ex, DM_OUT, ao, M, C);
    // (producers of the shadow: the projections that run the f16 kernels -- f16 or X2 -- where the selection picks the weights-in-registers kernel)
    { Epi e1 = er; if (pl.out1 != LF_NATIVE) want_shadow(e1, pl.q2_sh, pl.q2, b.n2); run_linear(ex, b.out1, pl.out1 == LF_F16 ? ao16 : x2op(pl.out1, ao), (int)M, t, e1); }
    // cross-attention
    const LnIn i2 = ln_in(b.q2, b.q2_sh, pl.q2, b.n2, DM_XATTN);
    Epi e2q; e2q.cls = DM_XATTN; e2q.ln_stat = i2.stat;
    if (xa_fused) {      // the projection's waves run the 77-key attention on their own q tiles (hi / lo context images at split precision)
      e2q.rpb = HW; e2q.xa_k = kv_xa(si, j); e2q.xa_nctx = n_ctx_; e2q.xa_scale = 0.125f;
      if (pl.xattn == XA_SPLIT) e2q.xa_k_lo = kv_xa_lo(si, j);
      run_linear(ex, *i2.w, i2.a, (int)M, ao2, e2q);
    } else {
      const bool to_q32 = pl.q2 == LF_F16 && !q2_widen;
      const Act& qo = to_q32 ? q32 : q;
      if (i2.stat || to_q32) e2q.rpb = HW;      // (the other forms' launches select their kernel on the whole batch's rows)
      run_linear(ex, *i2.w, i2.a, (int)M, q2_widen ? ao2_16 : qo, e2q);
      if (q2_widen && !ex.dry) {
        if (q.dt == DT_HL) launch_f16_to_hl(ao2_16.p, ao2_16.ld, q.p, q.ld, M, C, ex.s);
        else launch_copy_rows(ao2_16.p, DT_F16, ao2_16.ld, q.p, q.dt, q.ld, (int)M, C, ex.s);
      }
      if (!i2.stat && pl.q2 != LF_F16) demote_lo(ex, DM_XATTN, q, M, C);
      if (hl_attn) attention_hl(ex, qo, kv_k(si, j), C, kv_vt(si, j), vt_ld_ctx_, ao2, B, w.heads, HW, n_ctx_, DM_XATTN);   // caches are HL16 (set_context)
      else attention(ex, qo, Act(kv_k(si, j), C, adt), kv_vt(si, j), vt_ld_ctx_, ao, B, w.heads, HW, n_ctx_);
    }
    demote_lo(ex, DM_OUT, ao, M, C);
    { Epi e2 = er; if (pl.out2 != LF_NATIVE) want_shadow(e2, pl.geglu_sh, pl.geglu, b.n3); run_linear(ex, b.out2, pl.out2 == LF_F16 ? ao2_16 : x2op(pl.out2, ao), (int)M, t, e2); }
    // feed-forward
    const LnIn ig = ln_in(b.geglu, b.geglu_sh, pl.geglu, b.n3, DM_GEGLU);
    Epi eg; eg.act = 1; eg.cls = DM_GEGLU; eg.ln_stat = ig.stat;
    if (ig.stat) eg.rpb = HW;
    const bool gg_widen = pl.ff != LF_F16 && geglu_widened(pl.geglu, ig, M);
    run_linear(ex, *ig.w, ig.a, (int)M, pl.ff == LF_F16 || gg_widen ? gg16 : gg, eg);
    if (gg_widen && !ex.dry) launch_f16_to_hl(gg16.p, gg16.ld, gg.p, gg.ld, M, 4 * C, ex.s);
    demote_lo(ex, DM_FF, gg, M, 4 * C);
    er.cls = DM_FF;
    { Epi ef = er; if (pl.ff != LF_NATIVE && j + 1 < w.blocks.size()) want_shadow(ef, pl.qkv_sh, pl.qkv, w.blocks[j + 1].n1); run_linear(ex, b.ff, pl.ff == LF_F16 ? gg16 : x2op(pl.ff, gg), (int)M, t, ef); }
  }
  Epi eo; eo.R = x; eo.rpb = HW; eo.cls = DM_CONV_PROJ;
  run_linear(ex, w.proj_out, hl_op(ex, w.proj_out, t, M, C, DM_CONV_PROJ, B), (int)M, x, eo);
  ex.act->reset(mk);
}

// ------------------------------------------------------------------------------------------ forward
// the skip / concat buffers of a run at top-level size H x W: every input entry writes the slice [cx, cx + C_skip) of the buffer its matching output entry
// reads, the previous output entry (the middle block for cat[0]) the slice [0, cx)
void UNet::alloc_skips(Exec& ex, int B, int H, int W, Skips& k) {
  const int n_in = (int)inp_.size(), n_out = (int)out_.size();
  SDXL_REQUIRE(n_in == n_out, "input/output block count mismatch");
  k.hs_h.assign(n_in, 0); k.hs_w.assign(n_in, 0);
  std::vector<int> hs_c(n_in);
  {
    int h = H, w = W;
    for (int i = 0; i < n_in; ++i) {
      const BlockDesc& d = inp_[i].d;
      if (d.kind == BK_DOWN) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
      k.hs_h[i] = h; k.hs_w[i] = w; hs_c[i] = d.c_out;
    }
  }
  k.cat.assign(n_out, Act());
  k.cx.assign(n_out, 0);
  for (int j = 0; j < n_out; ++j) {
    const int i = n_in - 1 - j;
    k.cx[j] = out_[j].d.c_in - hs_c[i];
    SDXL_REQUIRE(k.cx[j] > 0, "bad concat geometry");
    k.cat[j] = ex.alloc((size_t)B * k.hs_h[i] * k.hs_w[i], out_[j].d.c_in, ex.sdt);
  }
}

// one entry of the block plan, src -> dst, at the entry's own input resolution h x w (a Down entry writes (h - 1) / 2 + 1, an entry with an upsample
// convolution 2h x 2w); si: the index of its spatial transformer in execution order (st_list_ / kv_)
void UNet::run_entry(Exec& ex, int section, int index, const Act& src, const Act& dst, int B, int h, int w, int si, const Act* add) {
  if (section == SEC_INPUT) {
    const BlockW& b = inp_[index];
    const int cur_c = b.d.c_in;
    switch (b.d.kind) {
      case BK_CONV: {
        Epi e = tag_epi(DM_CONV_IO);
        if (add) e.R = *add;
        run_conv(ex, b.conv, hl_op(ex, b.conv, src, (size_t)B * h * w, cur_c, DM_CONV_IO, B), cur_c, ConvGeom{B, h, w, h, w, 3, 1, 1, 0}, dst, e);
        break;
      }
      case BK_DOWN: {
        const int h2 = (h - 1) / 2 + 1, w2 = (w - 1) / 2 + 1;
        run_conv(ex, b.conv, hl_op(ex, b.conv, src, (size_t)B * h * w, cur_c, DM_CONV_UPDOWN, B), cur_c, ConvGeom{B, h, w, h2, w2, 3, 2, 1, 0}, dst, tag_epi(DM_CONV_UPDOWN));
        break;
      }
      case BK_RES: res_block(ex, b.res, src, B, h, w, dst); break;
      case BK_REST: {
        Act d = dst;      // statistics of the ResBlock output for the transformer's GroupNorm (scratch outlives both calls)
        const size_t mkp = ex.act->mark();
        float* part = (float*)ex.act->alloc((size_t)B * h * w / 256 * b.d.c_out * 2 * sizeof(float) + 256);
        d.gn_part = res_block(ex, b.res, src, B, h, w, dst, part); d.gn_rt = h * w / 256;
        spatial_transformer(ex, b.st, si, d, B, h, w);
        ex.act->reset(mkp);
        break;
      }
      default: throw Error("unexpected input block kind");
    }
  } else if (section == SEC_MIDDLE) {      // (:480, :713-719)
    const size_t mk = ex.act->mark();
    Act m1 = ex.alloc((size_t)B * h * w, mid_res1_.d.c_out, ex.sdt);
    float* part = (float*)ex.act->alloc((size_t)B * h * w / 256 * mid_res1_.d.c_out * 2 * sizeof(float) + 256);
    m1.gn_part = res_block(ex, mid_res1_.res, src, B, h, w, m1, part); m1.gn_rt = h * w / 256;
    spatial_transformer(ex, mid_res1_.st, si, m1, B, h, w);
    m1.gn_part = nullptr;                 // the transformer rewrote m1 in place
    res_block(ex, mid_res2_.res, m1, B, h, w, dst);
    ex.act->reset(mk);
  } else if (section == SEC_OUTPUT) {
    const BlockW& b = out_[index];
    const bool up = b.d.kind == BK_RESTU || b.d.kind == BK_RESU;
    const size_t mk = ex.act->mark();
    Act dest = up ? ex.alloc((size_t)B * h * w, b.d.c_out, ex.sdt) : dst;
    if (b.d.kind == BK_REST || b.d.kind == BK_RESTU) {
      float* part = (float*)ex.act->alloc((size_t)B * h * w / 256 * b.d.c_out * 2 * sizeof(float) + 256);
      Act d = dest;
      d.gn_part = res_block(ex, b.res, src, B, h, w, dest, part); d.gn_rt = h * w / 256;
      spatial_transformer(ex, b.st, si, d, B, h, w);
    } else {
      res_block(ex, b.res, src, B, h, w, dest);
    }
    if (up) {   // Upsample::forward :742-752 -- nearest 2x folded into the conv weights (four 2x2-tap phase convolutions) or, where the shape has no such launch, fused into the conv gather
      Epi up_epi = tag_epi(DM_CONV_UPDOWN);
      up_epi.fold = true;      // (run_conv: only layers that carry folded weights -- the f16 engine's)
      run_conv(ex, b.conv, hl_op(ex, b.conv, dest, (size_t)B * h * w, b.d.c_out, DM_CONV_UPDOWN, B), b.d.c_out, ConvGeom{B, h, w, 2 * h, 2 * w, 3, 1, 1, 1}, dst, up_epi);
    }
    ex.act->reset(mk);
  } else {      // SEC_HEAD (:488-490)
    const int mc = cfg_.model_channels;
    const size_t mk = ex.act->mark();
    Act gn = ex.alloc((size_t)B * h * w, mc, ex.cdt);
    run_groupnorm(ex, norm_out_, src, B, h * w, gn, true);
    demote_lo(ex, DM_CONV_IO, gn, (size_t)B * h * w, mc);
    run_conv(ex, conv_out_, gn, mc, ConvGeom{B, h, w, h, w, 3, 1, 1, 0}, dst, tag_epi(DM_CONV_IO));
    ex.act->reset(mk);
  }
}

void UNet::run(Exec& ex, const float* t_dev, int t_stride, int b0, int nb) {
  // batch entries [b0, b0 + nb) of the plan: every per-entry buffer is addressed through these views
  const int B = nb, H = pH_, W = pW_;
  const int mc = cfg_.model_channels, emb = 4 * mc;
  float* temb = temb_ + (size_t)b0 * mc;
  float* g1 = g1_ + (size_t)b0 * emb;
  float* embv = emb_ + (size_t)b0 * emb;
  float* ebias = ebias_ + (size_t)b0 * emb_total_;
  const float* label_emb = label_emb_ ? label_emb_ + (size_t)b0 * emb : nullptr;
  void* in = (char*)in_ + (size_t)b0 * H * W * cfg_.in_channels * dt_size(input_dt());
  float* eps = eps_ + (size_t)b0 * H * W * cfg_.out_channels;
  ex.ebias = ebias; ex.b0 = b0;
  ex.gn_partial = gn_partial_ + (size_t)b0 * groupnorm_workspace_floats(1, 32);
  // --- embeddings (unet/mod.rs:458-468)
  if (!ex.dry) launch_timestep_embedding(t_dev + (size_t)b0 * t_stride, t_stride, temb, B, mc, ex.s);
  gemv(ex, lin1_t_, temb, mc, g1, emb, B, false, true);
  gemv(ex, lin2_t_, g1, emb, embv, emb, B, false, false, label_emb);
  gemv(ex, embcat_, embv, emb, ebias, emb_total_, B, true, false);
  if (control_) { run_control(ex, B, H, W, in); return; }

  // --- geometry of the skip / concat buffers
  Skips k;
  alloc_skips(ex, B, H, W, k);
  const std::vector<Act>& cat = k.cat;
  const std::vector<int>& cx = k.cx;
  const int n_in = (int)inp_.size(), n_out = (int)out_.size();
  auto has_st = [](const BlockW& b) { return b.d.kind == BK_REST || b.d.kind == BK_RESTU; };
  // --- input blocks (:474-477)
  Act cur(in, cfg_.in_channels, input_dt());
  int h = H, w = W;
  int si = 0;
  for (int i = 0; i < n_in; ++i) {
    const Act dest = cat[n_in - 1 - i].cols(cx[n_in - 1 - i]);
    run_entry(ex, SEC_INPUT, i, cur, dest, B, h, w, si);
    if (has_st(inp_[i])) ++si;
    if (inp_[i].d.kind == BK_DOWN) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
    cur = dest;
  }
  // --- middle block
  run_entry(ex, SEC_MIDDLE, 0, cur, cat[0].cols(0), B, h, w, si++);
  // --- skip residuals (ControlNet): scale * r into every skip half and the middle block's output, one launch over the plan's table
  if (res_key_ && !ex.dry) {
    SDXL_REQUIRE(res_table_ok_ && b0 == 0 && nb == pB_ && cat[0].p == res_dst_mid_, "skip residuals: the segment table does not describe this run");
    if (ex.prof) ex.prof->begin(Profiler::OTHER, 0.0, ex.s);
    launch_skip_add(res_table_, res_segs_, 1, res_chunks_, res_scale_, nullptr, 0, sdt_, ex.s);
    if (ex.prof) ex.prof->end(ex.s);
  }
  // --- output blocks (:483-486)
  Act last = ex.alloc((size_t)B * H * W, mc, ex.sdt);
  for (int j = 0; j < n_out; ++j) {
    run_entry(ex, SEC_OUTPUT, j, cat[j], j + 1 < n_out ? cat[j + 1].cols(0) : last, B, h, w, si);
    if (has_st(out_[j])) ++si;
    if (out_[j].d.kind == BK_RESTU || out_[j].d.kind == BK_RESU) { h *= 2; w *= 2; }
  }
  SDXL_REQUIRE(h == H && w == W, "UNet input height/width must be divisible by 2^(levels-1)");
  // --- out
  run_entry(ex, SEC_HEAD, 0, last, Act(eps, cfg_.out_channels, DT_F32), B, H, W, 0);
}

void UNet::ensure_plan(int B, int H, int W) {
  const bool split = split_cfg_ && B == 2;
  if (B == pB_ && H == pH_ && W == pW_ && split == plan_split_ && fuse_xattn_ == plan_xattn_ && gn_from_producer_ == plan_gn_) return;
  SDXL_REQUIRE(B >= 1 && B <= 8, "batch must be in 1..8");
  const int div = 1 << (cfg_.channel_mults.size() - 1);
  SDXL_REQUIRE(H >= div && W >= div && H % div == 0 && W % div == 0,
               "UNet input height/width must be divisible by 2^(levels-1)");
  if (graph_) { (void)hipGraphExecDestroy(graph_); graph_ = nullptr; }
  plan_runs_ = 0;
  warm_ = WarmSeq();
  res_table_ok_ = false;      // (the concat buffers move with the arena)
  hint_g_ = nullptr;          // (control mode: the hint features belong to a plan)
  pB_ = B; pH_ = H; pW_ = W;
  const int mc = cfg_.model_channels, emb = 4 * mc;
  auto persist = [&]() {
    in_ = act_.alloc((size_t)B * H * W * cfg_.in_channels * dt_size(input_dt()));
    eps_ = (float*)act_.alloc((size_t)B * H * W * cfg_.out_channels * sizeof(float));
    temb_ = (float*)act_.alloc((size_t)B * mc * sizeof(float));
    g1_ = (float*)act_.alloc((size_t)B * emb * sizeof(float));
    emb_ = (float*)act_.alloc((size_t)B * emb * sizeof(float));
    ebias_ = (float*)act_.alloc((size_t)B * emb_total_ * sizeof(float));
    gn_partial_ = (float*)act_.alloc(groupnorm_workspace_floats(B, 32) * sizeof(float));
    tconv_ = (float*)act_.alloc(8 * sizeof(float));
    if (control_) {      // the residual tensors: fixed addresses for the plan (the controlled UNet's segment table and both graphs hold them)
      ctl_res_.clear(); ctl_res_bytes_.clear();
      for (const SkipShape& k : skip_shapes(cfg_, H, W)) {
        ctl_res_bytes_.push_back((size_t)B * k.C * k.h * k.w * dt_size(sdt_));
        ctl_res_.push_back(act_.alloc(ctl_res_bytes_.back()));
      }
    }
    if (attn16_) {   // cross-workgroup key split of the (f16) self-attention: workspace + tickets per chain, sized for the largest level
      size_t wsb = 0, cnt = 0;
      { int h = H, w = W;
        for (size_t lv = 0; lv < cfg_.channel_mults.size(); ++lv) {
          const int heads = cfg_.model_channels * cfg_.channel_mults[lv] / cfg_.n_head_channels;
          if (lv < cfg_.transformer_depths.size() && cfg_.transformer_depths[lv] > 0) {      // (levels without a SpatialTransformer run no attention)
            wsb = std::max(wsb, attention_xsplit_ws_bytes(B, heads, h * w)); cnt = std::max(cnt, attention_xsplit_counters(B, heads, h * w));
          }
          h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1;
        } }
      attn_xcnt_bytes_ = cnt * sizeof(unsigned);
      attn_xws_[1] = nullptr; attn_xcnt_[1] = nullptr;
      for (int c = 0; c < (split ? 2 : 1); ++c) {
        attn_xws_[c] = (float*)act_.alloc(wsb + 256);
        attn_xcnt_[c] = (unsigned*)act_.alloc(attn_xcnt_bytes_ + 256);
      }
    }
    if (cdt_ == DT_F16 || cdt_ == DT_HL) {   // split-K slabs + counters: chain 0 (and the second split-CFG chain)
      skws_bytes_ = igemm_splitk_ws_bytes(B, 1024, 1536);
      skws_[1] = nullptr; skcnt_[1] = nullptr;
      for (int c = 0; c < (split ? 2 : 1); ++c) {   // the second set only exists for the second split-CFG chain
        skws_[c] = (float*)act_.alloc(skws_bytes_);
        skcnt_[c] = (unsigned*)act_.alloc(kSplitkCounters * sizeof(unsigned));
      }
    }
  };
  // dry run for the peak, then the real arena
  act_.dry = true; act_.off = 0; act_.peak = 0;
  persist();
  Exec ex; ex.dry = true; ex.cdt = cdt_; ex.sdt = sdt_; ex.act = &act_;
  const size_t m = act_.mark();
  const bool had_kv = !kv_.empty();
  if (!had_kv) {   // plan built before set_context: fake cache entries for the dry run
    kv_.assign(st_list_.size(), std::vector<KV>());
    for (size_t i = 0; i < st_list_.size(); ++i) kv_[i].assign(st_list_[i]->blocks.size(), KV());
  }
  run(ex, nullptr, 0, 0, B);
  if (split) {   // scratch peak of one batch-1 chain -> the second chain's own arena
    act2_.dry = true; act2_.off = 0; act2_.peak = 0;
    Exec e2; e2.dry = true; e2.cdt = cdt_; e2.sdt = sdt_; e2.act = &act2_;
    run(e2, nullptr, 0, 1, 1);
    const size_t peak2 = act2_.peak;
    act2_.dry = false;
    act2_.reserve(peak2 + 4096);
    act2_.off = 0; act2_.peak = 0;
    if (!s2_) {
      SDXL_HIP(hipStreamCreateWithFlags(&s2_, hipStreamNonBlocking));
      SDXL_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
      SDXL_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
    }
  }
  plan_split_ = split;
  plan_xattn_ = fuse_xattn_;
  plan_gn_ = gn_from_producer_;
  if (!had_kv) kv_.clear();
  act_.reset(m);
  const size_t peak = act_.peak;
  act_.dry = false;
  act_.reserve(peak + 4096);
  act_.off = 0; act_.peak = 0;
  persist();
  for (int c = 0; c < 2; ++c) if (skcnt_[c]) SDXL_HIP(hipMemset(skcnt_[c], 0, kSplitkCounters * sizeof(unsigned)));   // armed once
  for (int c = 0; c < (split ? 2 : 1); ++c) if (attn_xcnt_[c] && attn16_) SDXL_HIP(hipMemset(attn_xcnt_[c], 0, attn_xcnt_bytes_));
  // a control net's residual buffers start as zeros, not as what the allocation held: a reader in front of the first forward sees numbers
  for (size_t i = 0; i < ctl_res_.size() && control_; ++i) SDXL_HIP(hipMemset(ctl_res_[i], 0, ctl_res_bytes_[i]));
}

void* UNet::unet_in(int B, int H, int W) { ensure_plan(B, H, W); return in_; }

void UNet::forward(int B, int H, int W, const float* t_dev, int t_stride, hipStream_t s) {
  ensure_plan(B, H, W);
  SDXL_REQUIRE(ctx_B_ == B && !kv_.empty(), "set_context must be called with the same batch before forward");
  SDXL_REQUIRE(label_valid_, "set_context must be called again before forward: a single-entry run (sdxl_unet_block) replaced the context and left no label embedding");
  prepare_residuals();
  Exec ex; ex.s = s; ex.cdt = cdt_; ex.sdt = sdt_; ex.act = &act_; ex.gn_partial = gn_partial_; ex.demote = demote_mask_;
  ex.splitk_ws = skws_[0]; ex.splitk_ws_bytes = skws_bytes_; ex.splitk_cnt = skcnt_[0];
  if (attn16_) { ex.attn_xws = attn_xws_[0]; ex.attn_xcnt = attn_xcnt_[0]; }
  // weight warming (f16 engine, batched chain): the plan's first forward records the GEMM sequence, every later one replays it
  const bool warming = cdt_ == DT_F16 && !plan_split_ && igemm_warm_enabled();
  if (warming) { ex.warm = &warm_; if (!warm_.ready) { warm_.seq.clear(); warm_.recording = true; } }
  const size_t m = act_.mark();
  // one batched chain, or (split-CFG) entry 0 on s and entry 1 on the side stream between a fork and a join event
  auto go = [&]() {
    warm_.pos = 0;
    if (!plan_split_) { run(ex, t_dev, t_stride, 0, B); if (warm_.recording) warm_.finish(); return; }
    Exec e2; e2.s = s2_; e2.cdt = cdt_; e2.sdt = sdt_; e2.act = &act2_; e2.demote = demote_mask_;
    e2.splitk_ws = skws_[1]; e2.splitk_ws_bytes = skws_bytes_; e2.splitk_cnt = skcnt_[1];
    if (attn16_) { e2.attn_xws = attn_xws_[1]; e2.attn_xcnt = attn_xcnt_[1]; }
    act2_.off = 0;
    ex.fork_ev = ev_fork_; ex.fork_after = split_offset_; ex.launches = 0;
    if (ex.fork_after <= 0) SDXL_HIP(hipEventRecord(ev_fork_, s));
    run(ex, t_dev, t_stride, 0, 1);
    if (ex.fork_after > 0 && ex.launches < ex.fork_after) SDXL_HIP(hipEventRecord(ev_fork_, s));   // offset beyond the chain
    ex.fork_ev = nullptr;
    SDXL_HIP(hipStreamWaitEvent(s2_, ev_fork_, 0));
    run(e2, t_dev, t_stride, 1, 1);
    SDXL_HIP(hipEventRecord(ev_join_, s2_));
    SDXL_HIP(hipStreamWaitEvent(s, ev_join_, 0));
  };
  if (use_graph_ && graph_ && (graph_t_ != t_dev || graph_ts_ != t_stride || graph_off_ != split_offset_ || graph_warm_ != warming || graph_demote_ != demote_mask_ ||
                               graph_res_key_ != res_key_ || graph_hint_ != hint_g_)) {
    (void)hipGraphExecDestroy(graph_); graph_ = nullptr;
  }
  if (use_graph_ && !graph_ && plan_runs_ >= 1) {
    // capture the whole forward (~1.3k launches) once; replay costs one launch per forward
    hipGraph_t g = nullptr;
    // the cross-workgroup tickets (attention key halves, split-K) re-arm themselves at the end of every launch; a forward that was torn down
    // half way (device error, cancelled capture) would leave them armed wrongly for good -- re-zero them whenever a graph is (re)captured
    for (int c = 0; c < 2; ++c) {
      if (attn_xcnt_[c] && attn_xcnt_bytes_) SDXL_HIP(hipMemsetAsync(attn_xcnt_[c], 0, attn_xcnt_bytes_, s));
      if (skcnt_[c]) SDXL_HIP(hipMemsetAsync(skcnt_[c], 0, kSplitkCounters * sizeof(unsigned), s));
    }
    SDXL_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    try { go(); } catch (...) { (void)hipStreamEndCapture(s, &g); if (g) (void)hipGraphDestroy(g); act_.reset(m); throw; }
    SDXL_HIP(hipStreamEndCapture(s, &g));
    SDXL_HIP(hipGraphInstantiate(&graph_, g, nullptr, nullptr, 0));
    SDXL_HIP(hipGraphDestroy(g));
    graph_t_ = t_dev; graph_ts_ = t_stride; graph_off_ = split_offset_; graph_warm_ = warming; graph_demote_ = demote_mask_; graph_res_key_ = res_key_; graph_hint_ = hint_g_;
    act_.reset(m);
  }
  if (use_graph_ && graph_) {
    SDXL_HIP(hipGraphLaunch(graph_, s));
  } else {
    go();
    act_.reset(m);
  }
  ++plan_runs_;
}

void UNet::profile(int B, int H, int W, float ms[Profiler::NCLS], int launches[Profiler::NCLS],
                   double flops[Profiler::NCLS], hipStream_t s) {
  ensure_plan(B, H, W);
  SDXL_REQUIRE(ctx_B_ == B && !kv_.empty(), "set_context must be called with the same batch before profile");
  SDXL_REQUIRE(label_valid_, "set_context must be called again before profile: a single-entry run (sdxl_unet_block) replaced the context and left no label embedding");
  prepare_residuals();
  const float t500[8] = {500.f, 500.f, 500.f, 500.f, 500.f, 500.f, 500.f, 500.f};
  SDXL_HIP(hipMemcpyAsync(tconv_, t500, sizeof(t500), hipMemcpyHostToDevice, s));
  SDXL_HIP(hipStreamSynchronize(s));
  Profiler prof;
  Exec ex; ex.s = s; ex.cdt = cdt_; ex.sdt = sdt_; ex.act = &act_; ex.gn_partial = gn_partial_; ex.prof = &prof; ex.demote = demote_mask_;
  ex.splitk_ws = skws_[0]; ex.splitk_ws_bytes = skws_bytes_; ex.splitk_cnt = skcnt_[0];
  if (attn16_) { ex.attn_xws = attn_xws_[0]; ex.attn_xcnt = attn_xcnt_[0]; }
  const size_t m = act_.mark();
  run(ex, tconv_, 1, 0, B);   // always the batched chain: per-launch events need one stream
  act_.reset(m);
  prof.collect(ms, launches, flops);
}

// the same eager chain WITHOUT the per-launch events, bracketed by one event pair: what the launches of profile() take when nobody measures them one
// by one -- (sum of profile()'s class times - this) / launches is the event overhead a bracketed launch carries (bench.py's calibration)
float UNet::eager_ms(int B, int H, int W, hipStream_t s) {
  ensure_plan(B, H, W);
  SDXL_REQUIRE(ctx_B_ == B && !kv_.empty(), "set_context must be called with the same batch before eager_ms");
  SDXL_REQUIRE(label_valid_, "set_context must be called again before eager_ms: a single-entry run (sdxl_unet_block) replaced the context and left no label embedding");
  prepare_residuals();
  const float t500[8] = {500.f, 500.f, 500.f, 500.f, 500.f, 500.f, 500.f, 500.f};
  SDXL_HIP(hipMemcpyAsync(tconv_, t500, sizeof(t500), hipMemcpyHostToDevice, s));
  SDXL_HIP(hipStreamSynchronize(s));
  hipEvent_t a, b;
  SDXL_HIP(hipEventCreate(&a)); SDXL_HIP(hipEventCreate(&b));
  float best = 0.f;
  for (int rep = 0; rep < 3; ++rep) {
    Exec ex; ex.s = s; ex.cdt = cdt_; ex.sdt = sdt_; ex.act = &act_; ex.gn_partial = gn_partial_; ex.demote = demote_mask_;
    ex.splitk_ws = skws_[0]; ex.splitk_ws_bytes = skws_bytes_; ex.splitk_cnt = skcnt_[0];
    if (attn16_) { ex.attn_xws = attn_xws_[0]; ex.attn_xcnt = attn_xcnt_[0]; }
    const size_t m = act_.mark();
    SDXL_HIP(hipEventRecord(a, s));
    run(ex, tconv_, 1, 0, B);
    SDXL_HIP(hipEventRecord(b, s));
    act_.reset(m);
    SDXL_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    SDXL_HIP(hipEventElapsedTime(&ms, a, b));
    if (rep == 0 || ms < best) best = ms;
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  return best;
}

void UNet::run_block(int section, int index, const float* x, const float* emb, const float* context, int n_ctx, int B, int c_in, int h, int w, float* out,
                     int64_t out_shape[4], hipStream_t s) {
  auto require = [](bool ok, const char* msg) { if (!ok) throw InvalidArgumentError(std::string("unet block: ") + msg); };
  constexpr int kMaxTop = 256;      // top-level latent height / width (a 2048-pixel image): larger plans are refused here, not by the arena
  const int n_in = (int)inp_.size(), n_out = (int)out_.size(), mc = cfg_.model_channels;
  require(section >= SEC_INPUT && section <= SEC_HEAD, "section must be 0 (input), 1 (middle), 2 (output) or 3 (head)");
  require(index >= 0 && index < (section == SEC_INPUT ? n_in : section == SEC_OUTPUT ? n_out : 1), "index outside the block plan");
  require(B >= 1 && B <= 8 && h >= 1 && w >= 1 && h <= kMaxTop && w <= kMaxTop && n_ctx >= 1, "batch must be in 1..8, h and w in 1..256");
  auto has_st = [](const BlockW& b) { return b.d.kind == BK_REST || b.d.kind == BK_RESTU; };
  // the entry's level (Down entries before it), its transformer's index and its widths in the plan
  const int last_in = section == SEC_INPUT ? index : section == SEC_MIDDLE ? n_in : section == SEC_OUTPUT ? n_in - 1 - index : 0;      // input entries [0, last_in) run before the entry's source exists
  int level = 0, si = 0;
  for (int i = 0; i < n_in; ++i) {
    if (i < (section == SEC_OUTPUT ? last_in + 1 : last_in) && inp_[i].d.kind == BK_DOWN) ++level;
    if ((section != SEC_INPUT || i < index) && has_st(inp_[i])) ++si;
  }
  if (section == SEC_OUTPUT) { ++si; for (int j = 0; j < index; ++j) if (has_st(out_[j])) ++si; }
  const BlockDesc& d = section == SEC_INPUT ? inp_[index].d : section == SEC_MIDDLE ? mid_res1_.d : out_[section == SEC_OUTPUT ? index : 0].d;
  const int want_c = section == SEC_HEAD ? mc : d.c_in, c_out = section == SEC_HEAD ? cfg_.out_channels : d.c_out;
  require(c_in == want_c, "c_in is not the entry's input width");
  const int H = h << level, W = w << level;
  const int div = 1 << (cfg_.channel_mults.size() - 1);
  require(H <= kMaxTop && W <= kMaxTop, "the top-level size the entry's level implies exceeds 256 x 256");
  require(H % div == 0 && W % div == 0, "no forward has this size at the entry's level (top-level height / width divisible by 2^(levels-1))");
  int ho = h, wo = w;
  if (section == SEC_INPUT && d.kind == BK_DOWN) { ho = (h - 1) / 2 + 1; wo = (w - 1) / 2 + 1; }
  if (section == SEC_OUTPUT && (d.kind == BK_RESTU || d.kind == BK_RESU)) { ho = 2 * h; wo = 2 * w; }
  if (out_shape) { out_shape[0] = B; out_shape[1] = c_out; out_shape[2] = ho; out_shape[3] = wo; }
  if (!out) return;
  require(x && emb && context, "null tensor");
  ensure_plan(B, H, W);
  set_context(context, n_ctx, nullptr, B, s);
  Exec ex; ex.s = s; ex.cdt = cdt_; ex.sdt = sdt_; ex.act = &act_; ex.gn_partial = gn_partial_; ex.demote = demote_mask_;
  ex.splitk_ws = skws_[0]; ex.splitk_ws_bytes = skws_bytes_; ex.splitk_cnt = skcnt_[0];
  if (attn16_) { ex.attn_xws = attn_xws_[0]; ex.attn_xcnt = attn_xcnt_[0]; }
  ex.ebias = ebias_; ex.b0 = 0;
  const size_t m = act_.mark();
  try {
    // every ResBlock's time-embedding bias, as run computes it: the entry reads its own emb_off slice
    SDXL_HIP(hipMemcpyAsync(emb_, emb, (size_t)B * 4 * mc * sizeof(float), hipMemcpyDeviceToDevice, s));
    gemv(ex, embcat_, emb_, 4 * mc, ebias_, emb_total_, B, true, false);
    Skips k;
    alloc_skips(ex, B, H, W, k);
    const Act last = ex.alloc((size_t)B * H * W, mc, ex.sdt);
    const int before = last_in - (section == SEC_OUTPUT ? 0 : 1);      // the input entry that leaves the resolution this entry runs at
    SDXL_REQUIRE(section == SEC_HEAD || before < 0 || (k.hs_h[before] == h && k.hs_w[before] == w), "unet block: level geometry");
    Act src, dst;
    switch (section) {
      case SEC_INPUT:
        src = index == 0 ? Act(in_, cfg_.in_channels, input_dt()) : k.cat[n_in - index].cols(k.cx[n_in - index]);
        dst = k.cat[n_in - 1 - index].cols(k.cx[n_in - 1 - index]);
        break;
      case SEC_MIDDLE: src = k.cat[0].cols(k.cx[0]); dst = k.cat[0].cols(0); break;
      case SEC_OUTPUT: src = k.cat[index]; dst = index + 1 < n_out ? k.cat[index + 1].cols(0) : last; break;
      default: src = last; dst = Act(eps_, cfg_.out_channels, DT_F32);
    }
    launch_nchw_to_nhwc(x, c_in * h * w, src.p, src.dt, B, c_in, h * w, src.ld, 1.0f, s);
    run_entry(ex, section, index, src, dst, B, h, w, si);
    launch_nhwc_to_nchw(dst.p, dst.dt, dst.ld, out, B, c_out, ho * wo, 1.0f, s);
  } catch (...) { act_.reset(m); throw; }
  act_.reset(m);
}

// ------------------------------------------------------------------------------------------ skip residuals (ControlNet)
std::vector<UNet::SkipShape> UNet::skip_shapes(const UNetCfg& cfg, int H, int W) {
  std::vector<BlockDesc> inp, out; BlockDesc mid;
  unet_block_plan(cfg, inp, mid, out);
  const int div = 1 << (cfg.channel_mults.size() - 1);
  if (H < div || W < div || H % div != 0 || W % div != 0)
    throw InvalidArgumentError("skip residuals: the latent height and width must be positive multiples of 2^(levels-1)");
  std::vector<SkipShape> v;
  int h = H, w = W;
  for (const BlockDesc& d : inp) {
    if (d.kind == BK_DOWN) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
    SkipShape s; s.C = d.c_out; s.h = h; s.w = w;
    v.push_back(s);
  }
  SkipShape m; m.C = mid.c_out; m.h = h; m.w = w;
  v.push_back(m);
  return v;
}
const char* UNet::residuals_refused() const {
  if (split_cfg_) return "skip residuals (ControlNet) cannot be combined with set_split_cfg: disable split CFG first";
  if (mix_ != 0 || mix_mode_ || (cdt_ == DT_F16 && sdt_ != DT_F16))
    return "skip residuals (ControlNet) take SDXL_DTYPE_F32, SDXL_DTYPE_F16 or SDXL_DTYPE_F32_SPLIT handles, not SDXL_DTYPE_F16_F32RES, the SDXL_DTYPE_F32_SPLIT_MIX* modes or SDXL_DTYPE_F32_SPLIT_F16W";
  return nullptr;
}
void UNet::clear_residuals() { res_key_ = 0; res_table_ok_ = false; }
void UNet::stage_residuals(const float* residuals, int B, int H, int W, float scale, hipStream_t s) {
  const std::vector<SkipShape> sh = skip_shapes(cfg_, H, W);
  const size_t es = dt_size(sdt_);
  if (!(res_key_ && res_B_ == B && res_H_ == H && res_W_ == W)) {      // new buffers: a captured graph holds the old addresses -> new key
    size_t bytes = 4096 + round_up(sh.size() * sizeof(SkipSeg), 256);
    for (const SkipShape& k : sh) bytes += round_up((size_t)B * k.C * k.h * k.w * es, 256);
    res_arena_.reserve(bytes);
    res_arena_.off = 0;
    res_scale_ = (float*)res_arena_.alloc(sizeof(float));
    res_table_ = (SkipSeg*)res_arena_.alloc(sh.size() * sizeof(SkipSeg));
    res_src_.clear();
    for (const SkipShape& k : sh) res_src_.push_back(res_arena_.alloc((size_t)B * k.C * k.h * k.w * es));
    res_B_ = B; res_H_ = H; res_W_ = W;
    res_key_ = ++res_serial_;
    res_table_ok_ = false;
  }
  const float* p = residuals;
  for (size_t i = 0; i < sh.size(); ++i) {
    const SkipShape& k = sh[i];
    launch_nchw_to_nhwc(p, k.C * k.h * k.w, const_cast<void*>(res_src_[i]), sdt_, B, k.C, k.h * k.w, k.C, 1.0f, s);
    p += (size_t)B * k.C * k.h * k.w;
  }
  unsigned bits; std::memcpy(&bits, &scale, sizeof(bits));
  SDXL_HIP(hipMemsetD32Async((hipDeviceptr_t)res_scale_, (int)bits, 1, s));
}
void UNet::prepare_residuals() {
  if (!res_key_ || res_table_ok_) return;
  SDXL_REQUIRE(res_B_ == pB_ && res_H_ == pH_ && res_W_ == pW_ && !plan_split_, "skip residuals were attached for another plan");
  Exec e; e.cdt = cdt_; e.sdt = sdt_; e.act = &act_;
  Skips k;
  const size_t m = act_.mark();      // run's first allocation: the same addresses every forward of this plan
  alloc_skips(e, pB_, pH_, pW_, k);
  act_.reset(m);
  const int n_in = (int)inp_.size();
  SDXL_REQUIRE((int)res_src_.size() == n_in + 1, "skip residuals: source count");
  std::vector<SkipSeg> t(n_in + 1);
  for (int i = 0; i < n_in; ++i) {
    const int j = n_in - 1 - i;
    const Act d = k.cat[j].cols(k.cx[j]);
    t[i] = SkipSeg{d.p, {res_src_[i]}, (long long)d.ld, pB_ * k.hs_h[i] * k.hs_w[i], inp_[i].d.c_out, 0ull};
  }
  t[n_in] = SkipSeg{k.cat[0].p, {res_src_[n_in]}, (long long)k.cat[0].ld, pB_ * k.hs_h[n_in - 1] * k.hs_w[n_in - 1], mid_res1_.d.c_out, 0ull};
  if (const char* bad = skip_table_check(t.data(), n_in + 1, 1, 0, sdt_, &res_chunks_)) throw InvalidArgumentError(bad);
  SDXL_HIP(hipMemcpy(res_table_, t.data(), t.size() * sizeof(SkipSeg), hipMemcpyHostToDevice));
  res_segs_ = n_in + 1;
  res_dst_mid_ = k.cat[0].p;
  res_table_ok_ = true;
}
void UNet::forward_residuals_nchw(const float* x, const int* timesteps, const float* context, int n_ctx, const float* label, int B, int H, int W,
                                  const float* residuals, float scale, float* out, hipStream_t s) {
  if (!residuals) { forward_nchw(x, timesteps, context, n_ctx, label, B, H, W, out, s); return; }
  if (const char* bad = residuals_refused()) throw InvalidArgumentError(bad);
  if (!std::isfinite(scale)) throw InvalidArgumentError("skip residuals: the scale must be finite");
  if (B < 1 || B > 8) throw InvalidArgumentError("skip residuals: batch must be in 1..8");
  (void)skip_shapes(cfg_, H, W);      // (the size check, before anything is planned)
  ensure_plan(B, H, W);
  stage_residuals(residuals, B, H, W, scale, s);
  set_context(context, n_ctx, label, B, s);
  launch_nchw_to_nhwc(x, cfg_.in_channels * H * W, in_, input_dt(), B, cfg_.in_channels, H * W, cfg_.in_channels, 1.0f, s);
  launch_i32_to_f32(timesteps, tconv_, B, s);
  forward(B, H, W, tconv_, 1, s);
  launch_nhwc_to_nchw(eps_, DT_F32, cfg_.out_channels, out, B, cfg_.out_channels, H * W, 1.0f, s);
}

// ------------------------------------------------------------------------------------------ control net (a UNet in control mode)
// control forward behind the embeddings: every input entry into a dense stream tensor of its own (entry 0: + the hint features, the residual input of
// its convolution), its 1x1 convolution into the plan's residual buffer; then the middle block and its 1x1 convolution
void UNet::run_control(Exec& ex, int B, int H, int W, void* in) {
  SDXL_REQUIRE(ex.dry || hint_g_, "control net: set_hint must be called before forward");
  const int n_in = (int)inp_.size(), mc = cfg_.model_channels;
  SDXL_REQUIRE((int)zero_.size() == n_in && (int)ctl_res_.size() == n_in + 1, "control net: residual buffers");
  const Act g(hint_g_, mc, ex.sdt);
  Act cur(in, cfg_.in_channels, input_dt());
  int h = H, w = W, si = 0;
  const size_t mk = ex.act->mark();
  auto one_by_one = [&](const Lin& l, const Act& x, int C, void* dst) {
    run_conv(ex, l, hl_op(ex, l, x, (size_t)B * h * w, C, DM_CONV_SKIP, B), C, ConvGeom{B, h, w, h, w, 1, 1, 0, 0}, Act(dst, C, ex.sdt), tag_epi(DM_CONV_SKIP));
  };
  for (int i = 0; i < n_in; ++i) {
    const BlockDesc& d = inp_[i].d;
    const int ho = d.kind == BK_DOWN ? (h - 1) / 2 + 1 : h, wo = d.kind == BK_DOWN ? (w - 1) / 2 + 1 : w;
    const Act dest = ex.alloc((size_t)B * ho * wo, d.c_out, ex.sdt);
    run_entry(ex, SEC_INPUT, i, cur, dest, B, h, w, si, i == 0 ? &g : nullptr);
    if (d.kind == BK_REST) ++si;
    h = ho; w = wo;
    one_by_one(zero_[i], dest, d.c_out, ctl_res_[i]);
    cur = dest;
  }
  const Act m = ex.alloc((size_t)B * h * w, mid_res1_.d.c_out, ex.sdt);
  run_entry(ex, SEC_MIDDLE, 0, cur, m, B, h, w, si);
  one_by_one(mid_out_, m, mid_res1_.d.c_out, ctl_res_[n_in]);
  ex.act->reset(mk);
}
void UNet::set_hint(const float* hint, int n, int B, int H, int W, hipStream_t s) {
  SDXL_REQUIRE(control_, "set_hint: not a control net");
  if (!hint || n < 1 || (B != n && B != 2 * n)) throw InvalidArgumentError("control net: the batch must be the hint's n or 2 n (the CFG pair)");
  ensure_plan(B, H, W);
  const int mc = cfg_.model_channels, H8 = 8 * H, W8 = 8 * W;
  const int* hc = ccfg_.hint_channels;
  const int ch[9] = {ccfg_.hint_in, hc[0], hc[0], hc[1], hc[1], hc[2], hc[2], hc[3], mc};
  const size_t g_bytes = (size_t)n * H * W * mc * dt_size(sdt_);
  // the eight convolutions with a SiLU launch between them, every layer's output kept: once over a dry arena for the size, then for real
  auto pass = [&](Exec& ex) {
    void* g = ex.act->alloc((B / n) * g_bytes);
    if (!ex.dry) SDXL_HIP(hipMemsetAsync(g, 0, (B / n) * g_bytes, s));      // (zeros under the convolutions' writes, not what the allocation held)
    Act x = ex.alloc((size_t)n * H8 * W8, ch[0], input_dt());
    if (!ex.dry) launch_nchw_to_nhwc(hint, ch[0] * H8 * W8, x.p, x.dt, n, ch[0], H8 * W8, ch[0], 1.0f, s);
    int h = H8, w = W8;
    for (int k = 0; k < 8; ++k) {
      const int st = (k == 2 || k == 4 || k == 6) ? 2 : 1, ho = (h - 1) / st + 1, wo = (w - 1) / st + 1;
      const Act y = k == 7 ? Act(g, mc, ex.sdt) : ex.alloc((size_t)n * ho * wo, ch[k + 1], ex.sdt);
      run_conv(ex, hint_conv_[k], hl_operand(ex, hint_conv_[k], x, (size_t)n * h * w, ch[k], n), ch[k], ConvGeom{n, h, w, ho, wo, 3, st, 1, 0}, y);
      if (k < 7 && !ex.dry) launch_silu_inplace(y.p, y.dt, (size_t)n * ho * wo * ch[k + 1], s);
      x = y; h = ho; w = wo;
    }
    SDXL_REQUIRE(h == H && w == W, "control net: the hint must be 8 x the latent size");
    if (B == 2 * n && !ex.dry) SDXL_HIP(hipMemcpyAsync((char*)g + g_bytes, g, g_bytes, hipMemcpyDeviceToDevice, s));
    return g;
  };
  DeviceArena dry; dry.dry = true;
  Exec e0; e0.dry = true; e0.cdt = cdt_; e0.sdt = sdt_; e0.act = &dry;
  (void)pass(e0);
  hint_arena_.reserve(dry.peak + 4096);
  hint_arena_.off = 0;
  Exec ex; ex.s = s; ex.cdt = cdt_; ex.sdt = sdt_; ex.act = &hint_arena_;
  hint_g_ = pass(ex);
  hint_n_ = n; hint_B_ = B; hint_H_ = H; hint_W_ = W;
  if (graph_ && graph_hint_ != hint_g_) { (void)hipGraphExecDestroy(graph_); graph_ = nullptr; }      // (the arena moved: the graph holds the old address)
}
void UNet::embed_hint_nchw(const float* hint, int n, int H, int W, float* out, hipStream_t s) {
  if (!hint || !out) throw InvalidArgumentError("control net: null tensor");
  (void)skip_shapes(cfg_, H, W);
  set_hint(hint, n, n, H, W, s);
  launch_nhwc_to_nchw(hint_g_, sdt_, cfg_.model_channels, out, n, cfg_.model_channels, H * W, 1.0f, s);
}
void UNet::control_forward_nchw(const float* x, const int* timesteps, const float* context, int n_ctx, const float* label, const float* hint, int B, int H,
                                int W, float* residuals_out, hipStream_t s) {
  SDXL_REQUIRE(control_, "control forward: not a control net");
  if (B < 1 || B > 8) throw InvalidArgumentError("control net: batch must be in 1..8");
  const std::vector<SkipShape> sh = skip_shapes(cfg_, H, W);
  set_hint(hint, B, B, H, W, s);
  set_context(context, n_ctx, label, B, s);
  launch_nchw_to_nhwc(x, cfg_.in_channels * H * W, in_, input_dt(), B, cfg_.in_channels, H * W, cfg_.in_channels, 1.0f, s);
  launch_i32_to_f32(timesteps, tconv_, B, s);
  forward(B, H, W, tconv_, 1, s);
  float* o = residuals_out;
  for (size_t i = 0; i < sh.size(); ++i) {
    launch_nhwc_to_nchw(ctl_res_[i], sdt_, sh[i].C, o, B, sh[i].C, sh[i].h * sh[i].w, 1.0f, s);
    o += (size_t)B * sh[i].C * sh[i].h * sh[i].w;
  }
}
void UNet::forward_nchw(const float* x, const int* timesteps, const float* context, int n_ctx, const float* label, int B,
                        int H, int W, float* out, hipStream_t s) {
  SDXL_REQUIRE(!control_, "a control net has no UNet forward (sdxl_controlnet_forward)");
  clear_residuals();      // the plain entry: exactly the launches of a handle that never had residuals
  ensure_plan(B, H, W);
  set_context(context, n_ctx, label, B, s);
  launch_nchw_to_nhwc(x, cfg_.in_channels * H * W, in_, input_dt(), B, cfg_.in_channels, H * W, cfg_.in_channels, 1.0f, s);
  launch_i32_to_f32(timesteps, tconv_, B, s);
  forward(B, H, W, tconv_, 1, s);
  launch_nhwc_to_nchw(eps_, DT_F32, cfg_.out_channels, out, B, cfg_.out_channels, H * W, 1.0f, s);
}

}  // namespace sdxl
