// C ABI of the engine (include/sdxl_mi355.h): opaque handles, status codes + thread-local error text, never aborts.
// This file: contexts, debug knobs, parameter specs, the UNet / CLIP / Diffuser / VAE handles, sampling and the weight broadcast;
// the single-op and micro-benchmark entries are in capi_ops.hip.
#include "capi_internal.h"
#include "select_debug.h"
#include "upsample_fold.h"
#include <algorithm>
#include <cstring>

using namespace sdxl;

thread_local std::string sdxl::g_err;

namespace {
// every create entry: allocate the handle, let `make` construct the model into it, delete the handle if that throws
template <class H, class F> void create_handle(sdxl_ctx* ctx, H** out, F make) {
  std::unique_ptr<H> h(new H());
  h->ctx = ctx;
  make(*h);
  *out = h.release();
}
UNetCfg to_cfg(const sdxl_unet_config* c) {
  SDXL_REQUIRE(c != nullptr, "null config");
  SDXL_REQUIRE(c->n_levels >= 1 && c->n_levels <= 8, "n_levels out of range");
  UNetCfg u;
  u.adm_in_channels = c->adm_in_channels; u.in_channels = c->in_channels; u.out_channels = c->out_channels;
  u.model_channels = c->model_channels; u.n_head_channels = c->n_head_channels; u.context_dim = c->context_dim;
  u.is_refiner = c->is_refiner != 0;
  for (int i = 0; i < c->n_levels; ++i) { u.channel_mults.push_back(c->channel_mults[i]); u.transformer_depths.push_back(c->transformer_depths[i]); }
  SDXL_REQUIRE(u.model_channels > 0 && u.n_head_channels > 0 && u.context_dim > 0 && u.adm_in_channels > 0, "bad UNet config");
  return u;
}
ClipCfg to_ccfg(const sdxl_clip_config* c) {
  SDXL_REQUIRE(c != nullptr, "null config");
  ClipCfg k;
  k.n_vocab = c->n_vocab; k.n_state = c->n_state; k.embed_dim = c->embed_dim; k.n_head = c->n_head; k.n_ctx = c->n_ctx;
  k.n_layer = c->n_layer; k.quick_gelu = c->quick_gelu != 0;
  return k;
}
VaeCfg to_vcfg(const sdxl_vae_config* c) {
  SDXL_REQUIRE(c != nullptr, "null config");
  SDXL_REQUIRE(c->n_blocks >= 1 && c->n_blocks <= 8, "n_blocks out of range");
  VaeCfg v; v.enc.clear(); v.dec.clear();
  for (int i = 0; i < c->n_blocks; ++i) { v.enc.push_back({c->enc_in[i], c->enc_out[i]}); v.dec.push_back({c->dec_in[i], c->dec_out[i]}); }
  v.n_group = c->n_group; v.enc_out = c->enc_out_channels; v.scale_factor = c->scale_factor;
  SDXL_REQUIRE(v.n_group >= 1 && v.n_group <= 256, "n_group out of range (1..256)");
  for (int i = 0; i < c->n_blocks; ++i)
    for (int ch : {c->enc_in[i], c->enc_out[i], c->dec_in[i], c->dec_out[i]})
      SDXL_REQUIRE(ch > 0 && ch % v.n_group == 0 && ch % 8 == 0,
                   "The number of channels must be divisible by the number of groups (and by 8)");   // groupnorm/mod.rs:19-24
  return v;
}
void vae_create_impl(sdxl_ctx* ctx, const VaeCfg& vc, int cdt, WeightSource* dec, WeightSource* enc, sdxl_vae** out) {
  create_handle(ctx, out, [&](sdxl_vae& h) { h.v = new Vae(vc, cdt, dec, enc, ctx->stream); });
}
template <class Source, class T>      // FlatSource over fp32 buffers, FlatSourceF16 over IEEE-f16 ones
void vae_create_flat(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, const T* dec_w, const T* enc_w, sdxl_vae** out) {
  SDXL_REQUIRE(ctx && out && (dec_w || enc_w), "bad argument");
  use(ctx);
  int cdt; vae_dtype(dtype, cdt);
  const VaeCfg vc = to_vcfg(cfg);
  const std::vector<ParamSpec> ds = vae_decoder_param_specs(vc), es = vae_encoder_param_specs(vc);
  std::unique_ptr<Source> d, e;
  if (dec_w) d.reset(new Source(dec_w, ds));
  if (enc_w) e.reset(new Source(enc_w, es));
  vae_create_impl(ctx, vc, cdt, d.get(), e.get(), out);
}
int spec_out(const std::vector<ParamSpec>& specs, int index, const char** name, int* ndim, int64_t shape[4], int* kind,
             float* sc, float* mean) {
  if (index < 0 || index >= (int)specs.size()) return fail(SDXL_ERR_INVALID, "parameter index out of range");
  static thread_local std::string keep;
  const ParamSpec& p = specs[index];
  keep = p.name;
  if (name) *name = keep.c_str();
  if (ndim) *ndim = (int)p.shape.size();
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = i < (int)p.shape.size() ? p.shape[i] : 1;
  if (kind) *kind = p.kind;
  if (sc) *sc = p.scale;
  if (mean) *mean = p.mean;
  return SDXL_OK;
}
// the *_create_lora entries: argument errors are SDXL_ERR_INVALID before anything is built; then `make` gets the adapter source over the one base given
std::vector<LoraEntry> to_lora(const sdxl_lora_entry* e, int n) {
  std::vector<LoraEntry> v;
  for (int i = 0; i < n; ++i) { LoraEntry l; l.param_index = e[i].param_index; l.rank = e[i].rank; l.left = e[i].left; l.right = e[i].right; l.scale = e[i].scale; v.push_back(l); }
  return v;
}
template <class F>
int create_with_lora(sdxl_ctx* ctx, const sdxl_unet_config* cfg, const float* weights_flat, const uint16_t* weights_flat_f16, uint64_t seed,
                     const sdxl_lora_entry* entries, int n_entries, int flags, F make) {
  if (!ctx || !cfg) return fail(SDXL_ERR_INVALID, "null argument");
  if (weights_flat && weights_flat_f16) return fail(SDXL_ERR_INVALID, "lora: exactly one base -- weights_flat, weights_flat_f16, or both NULL for the synthetic seed");
  if (flags & ~SDXL_LORA_ROUND_F16) return fail(SDXL_ERR_INVALID, "lora: unknown flag bits (SDXL_LORA_ROUND_F16)");
  if (n_entries < 0 || (n_entries > 0 && !entries)) return fail(SDXL_ERR_INVALID, n_entries < 0 ? "lora: n_entries is negative" : "lora: entries is NULL");
  API_BEGIN
  const std::vector<ParamSpec> specs = unet_param_specs(to_cfg(cfg));
  const std::vector<LoraEntry> le = to_lora(entries, n_entries);
  const std::string bad = lora_check(specs, le.data(), n_entries);
  if (!bad.empty()) return fail(SDXL_ERR_INVALID, bad);
  use(ctx);
  std::unique_ptr<WeightSource> base;
  if (weights_flat) base.reset(new FlatSource(weights_flat, specs));
  else if (weights_flat_f16) base.reset(new FlatSourceF16(weights_flat_f16, specs));
  else base.reset(new SyntheticSource(seed));
  LoraSource src(*base, specs, le.data(), n_entries, flags);
  return make(src);
  API_END
}
}  // namespace

extern "C" {

const char* sdxl_last_error(void) { return g_err.c_str(); }
const char* sdxl_build_info(void) {
#ifdef SDXL_MEASURE
  return "sdxl_mi355 engine, HIP kernels for gfx950 (CDNA4, wave64, MFMA 32x32x16 f16 / 32x32x2 f32) [measure build: A/B variants + debug knobs]";
#else
  return "sdxl_mi355 engine, HIP kernels for gfx950 (CDNA4, wave64, MFMA 32x32x16 f16 / 32x32x2 f32)";
#endif
}

int sdxl_ctx_create(int device_id, sdxl_ctx** out) {
  API_BEGIN
  SDXL_REQUIRE(out != nullptr, "null out");
  int n = 0;
  SDXL_HIP(hipGetDeviceCount(&n));
  SDXL_REQUIRE(n > 0, "no HIP device visible: the MI355X engine has no CPU fallback");
  SDXL_REQUIRE(device_id >= 0 && device_id < n, "device id out of range");
  SDXL_HIP(hipSetDevice(device_id));
  sdxl_ctx* c = new sdxl_ctx();
  c->device = device_id;
  SDXL_HIP(hipStreamCreate(&c->stream));
  igemm_glds_init();
  *out = c;
  API_END
}
int sdxl_debug_set(const char* key, int value) {
  API_BEGIN
  SDXL_REQUIRE(key != nullptr, "null key");
  if (select_knob_set(key, value)) return SDXL_OK;      // the knobs of the kernel selection (SelectKnobs, select.cpp)
  else if (std::strcmp(key, "igemm_epilogue_staged") == 0) igemm_set_epilogue_staged(value);
  else if (std::strcmp(key, "hl_weights_exact") == 0) igemm_set_hl_weights_exact(value);
  else if (std::strcmp(key, "igemm_warm") == 0) igemm_set_warm(value);
  else if (std::strcmp(key, "splitk_wt") == 0) igemm_set_splitk_wt(value);
  else if (std::strcmp(key, "hl_demote") == 0) unet_set_hl_demote(value);
  else if (std::strcmp(key, "mix_classes") == 0) unet_set_mix_classes(value);
  else if (std::strcmp(key, "xattn_long") == 0) unet_set_xattn_long(value);
  else if (std::strcmp(key, "wreg_xcd2d") == 0) igemm_set_wreg_xcd2d(value);
  else if (std::strcmp(key, "upsample_fold") == 0) set_upsample_fold(value);
#ifdef SDXL_MEASURE
  else if (std::strcmp(key, "xa_vec64") == 0) igemm_set_xa_vec64(value);
  else if (std::strcmp(key, "no_cfg") == 0) g_debug_no_cfg = value != 0;
#endif
  else throw Error(std::string("unknown debug key ") + key);
  API_END
}
// host logic of the weight-warming schedule (WarmSeq::finish) on a synthetic launch sequence -- no device needed.  bytes[j] / host[j]: what entry j
// reads and whether its kernel can carry warming workgroups; warmed_by[j] receives the index of the entry that warms j (-1: nobody)
int sdxl_debug_warm_schedule(int n, const unsigned* bytes, const unsigned char* host, int* warmed_by) {
  API_BEGIN
  WarmSeq ws;
  for (int j = 0; j < n; ++j)
    ws.seq.push_back(WarmSeq::Item{reinterpret_cast<const void*>((uintptr_t)(j + 1) << 12), bytes[j], host[j] != 0, host[j] ? 14u << 20 : 0u, {nullptr, nullptr, nullptr}, {0u, 0u, 0u}});
  ws.finish();
  for (int j = 0; j < n; ++j) warmed_by[j] = -1;
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < 3; ++r)
      if (ws.seq[i].warm[r]) warmed_by[(int)(reinterpret_cast<uintptr_t>(ws.seq[i].warm[r]) >> 12) - 1] = i;
  API_END
}
// the weight fold of the upsample convolutions (upsample_fold.h) on host arrays -- no device needed: the arithmetic the model builders run per element
int sdxl_debug_upsample_fold(const float* weight, int cout, int cin, float* out) {
  API_BEGIN
  SDXL_REQUIRE(weight && out && cout > 0 && cin > 0, "bad argument");
  fold_upsample_weights(weight, out, (size_t)cout, (size_t)cin);
  API_END
}
// the layout pass of a model's weight arena (the loader over a dry arena and an empty source) -- no device needed
int sdxl_debug_weight_layout(const sdxl_unet_config* unet, const sdxl_vae_config* vae, const sdxl_clip_config* clip, int dtype, int option, size_t* bytes) {
  API_BEGIN
  SDXL_REQUIRE(bytes && (unet != nullptr) + (vae != nullptr) + (clip != nullptr) == 1, "weight layout: exactly one model description and a result");
  int cdt, sdt;
  if (unet) {
    dtypes(dtype, cdt, sdt);
    *bytes = UNet::weight_layout_bytes(to_cfg(unet), cdt, sdt, option < 0 ? mix_of(dtype) : option);
  } else if (vae) {
    vae_dtype(dtype, cdt);
    *bytes = Vae::weight_layout_bytes(to_vcfg(vae), cdt, true, option != 0);
  } else {
    no_mix(dtype); dtypes(dtype, cdt, sdt); no_split(cdt, "the CLIP text encoders");
    *bytes = ClipText::weight_layout_bytes(to_ccfg(clip), cdt);
  }
  API_END
}
// the kernel selection (select.cpp) on a described launch -- no device needed, the knobs come with the call
int sdxl_debug_igemm_select(const sdxl_igemm_case* c, const sdxl_select_knobs* knobs, sdxl_igemm_choice* out) {
  API_BEGIN
  SDXL_REQUIRE(c && knobs && out, "null argument");
  const IgemmParams p = select_debug_igemm(*c);
  const SelectKnobs k = select_debug_knobs(*knobs);
  *out = sdxl_igemm_choice{};
  out->gn_part_ok = igemm_gn_part_ok(p, k); out->wreg_selected = igemm_wreg_selected(p, k); out->wreg_xattn_selected = igemm_wreg_xattn_selected(p, k);
  const IgemmChoice s = igemm_select(p, c->compute_dt, k);
  out->family = s.family; out->bm = s.bm; out->bn = s.bn; out->ns = s.ns; out->wgm = s.wgm; out->nw = s.nw; out->elem = s.elem; out->a_elem = s.a_elem;
  out->xa = s.xa; out->xh = s.xh; out->tsw = s.tsw; out->s2 = s.s2; out->splitk = s.splitk; out->mode = s.mode; out->db = s.db; out->measure = s.measure;
  out->grid = s.grid; out->block = s.block; out->lds = s.lds;
  API_END
}
int sdxl_debug_attn_select(const sdxl_attn_case* c, const sdxl_select_knobs* knobs, sdxl_attn_choice* out) {
  API_BEGIN
  SDXL_REQUIRE(c && knobs && out, "null argument");
  const AttnChoice s = attn_select(select_debug_attn(*c), select_debug_knobs(*knobs));
  *out = sdxl_attn_choice{s.kernel, s.mix, s.big_heads, s.ns, s.elem, s.ko, s.grid_x, s.grid_y, s.block, s.lds};
  API_END
}
#ifdef SDXL_MEASURE
// measure builds only: device buffer [workgroups][waves][sdxl_debug_timeline_words()] unsigned that the s_memtime-stamped kernel
// variants (igemm_measure.hip, variants 135 / 136 / 145) dump their per-wave phase stamps into; null switches it off
int sdxl_debug_timeline(void* device_buf) {
  API_BEGIN
  igemm_set_timeline(device_buf);
  API_END
}
int sdxl_debug_timeline_words(void) { return igemm_timeline_words(); }
// device buffer [workgroups][8][8] unsigned for the coarse s_memtime stamps of the wide (GEGLU) kernel; null switches it off
int sdxl_debug_attn_timeline(void* device_buf) {
  API_BEGIN
  attention_set_timeline(device_buf);
  API_END
}
int sdxl_debug_wreg_timeline(void* device_buf) {
  API_BEGIN
  igemm_set_wreg_timeline(device_buf);
  API_END
}
int sdxl_debug_wide_timeline(void* device_buf) {
  API_BEGIN
  igemm_set_wide_timeline(device_buf);
  API_END
}
#endif
void sdxl_ctx_destroy(sdxl_ctx* c) {
  if (!c) return;
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}
int sdxl_ctx_synchronize(sdxl_ctx* c) {
  API_BEGIN
  use(c);
  SDXL_HIP(hipDeviceSynchronize());
  API_END
}

void sdxl_unet_config_base(sdxl_unet_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->adm_in_channels = 2816; c->in_channels = 4; c->out_channels = 4; c->model_channels = 320; c->n_levels = 3;
  const int m[3] = {1, 2, 4}, d[3] = {0, 2, 10};
  for (int i = 0; i < 3; ++i) { c->channel_mults[i] = m[i]; c->transformer_depths[i] = d[i]; }
  c->n_head_channels = 64; c->context_dim = 2048; c->is_refiner = 0;
}
void sdxl_unet_config_refiner(sdxl_unet_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->adm_in_channels = 2560; c->in_channels = 4; c->out_channels = 4; c->model_channels = 384; c->n_levels = 4;
  const int m[4] = {1, 2, 4, 4}, d[4] = {0, 4, 4, 4};
  for (int i = 0; i < 4; ++i) { c->channel_mults[i] = m[i]; c->transformer_depths[i] = d[i]; }
  c->n_head_channels = 64; c->context_dim = 1280; c->is_refiner = 1;
}
void sdxl_vae_config_default(sdxl_vae_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->n_blocks = 4;
  const int ei[4] = {128, 128, 256, 512}, eo[4] = {128, 256, 512, 512}, di[4] = {512, 512, 512, 256}, dn[4] = {512, 512, 256, 128};
  for (int i = 0; i < 4; ++i) { c->enc_in[i] = ei[i]; c->enc_out[i] = eo[i]; c->dec_in[i] = di[i]; c->dec_out[i] = dn[i]; }
  c->n_group = 32; c->enc_out_channels = 8; c->scale_factor = 0.13025;
}

int sdxl_unet_param_count(const sdxl_unet_config* cfg) {
  try { return (int)unet_param_specs(to_cfg(cfg)).size(); } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int sdxl_unet_param_spec(const sdxl_unet_config* cfg, int index, const char** name, int* ndim, int64_t shape[4], int* kind,
                         float* sc, float* mean) {
  API_BEGIN
  static thread_local std::vector<ParamSpec> cache; static thread_local sdxl_unet_config key;
  if (cache.empty() || std::memcmp(&key, cfg, sizeof(key)) != 0) { cache = unet_param_specs(to_cfg(cfg)); key = *cfg; }
  return spec_out(cache, index, name, ndim, shape, kind, sc, mean);
  API_END
}
int sdxl_vae_param_count(const sdxl_vae_config* cfg, int encoder) {
  try { return (int)(encoder ? vae_encoder_param_specs(to_vcfg(cfg)) : vae_decoder_param_specs(to_vcfg(cfg))).size(); }
  catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int sdxl_vae_param_spec(const sdxl_vae_config* cfg, int encoder, int index, const char** name, int* ndim, int64_t shape[4],
                        int* kind, float* sc, float* mean) {
  API_BEGIN
  const std::vector<ParamSpec> specs = encoder ? vae_encoder_param_specs(to_vcfg(cfg)) : vae_decoder_param_specs(to_vcfg(cfg));
  return spec_out(specs, index, name, ndim, shape, kind, sc, mean);
  API_END
}

// ---------------------------------------------------------------------------------------------- UNet
static int unet_create_impl(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, WeightSource& src, sdxl_unet** out) {
  SDXL_REQUIRE(ctx && out, "null argument");
  use(ctx);
  int cdt, sdt; dtypes(dtype, cdt, sdt);
  create_handle(ctx, out, [&](sdxl_unet& h) { h.u = new UNet(to_cfg(cfg), cdt, sdt, src, ctx->stream, mix_of(dtype)); });
  return SDXL_OK;
}
int sdxl_unet_create(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat, sdxl_unet** out) {
  API_BEGIN
  SDXL_REQUIRE(weights_flat != nullptr, "null weights");
  const std::vector<ParamSpec> specs = unet_param_specs(to_cfg(cfg));
  FlatSource src(weights_flat, specs);
  return unet_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
int sdxl_unet_create_f16(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const uint16_t* weights_flat_f16, sdxl_unet** out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && weights_flat_f16 != nullptr, "null argument");
  use(ctx);
  const std::vector<ParamSpec> specs = unet_param_specs(to_cfg(cfg));
  FlatSourceF16 src(weights_flat_f16, specs);
  return unet_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
int sdxl_unet_create_synthetic(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, uint64_t seed, sdxl_unet** out) {
  API_BEGIN
  SyntheticSource src(seed);
  return unet_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
int sdxl_lora_check(const sdxl_unet_config* cfg, const sdxl_lora_entry* entries, int n_entries) {
  if (!cfg) return fail(SDXL_ERR_INVALID, "null config");
  if (n_entries < 0 || (n_entries > 0 && !entries)) return fail(SDXL_ERR_INVALID, n_entries < 0 ? "lora: n_entries is negative" : "lora: entries is NULL");
  API_BEGIN
  const std::vector<LoraEntry> le = to_lora(entries, n_entries);
  const std::string bad = lora_check(unet_param_specs(to_cfg(cfg)), le.data(), n_entries);
  if (!bad.empty()) return fail(SDXL_ERR_INVALID, bad);
  API_END
}
int sdxl_unet_create_lora(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat, const uint16_t* weights_flat_f16,
                          uint64_t synthetic_seed, const sdxl_lora_entry* entries, int n_entries, int flags, sdxl_unet** out) {
  return create_with_lora(ctx, cfg, weights_flat, weights_flat_f16, synthetic_seed, entries, n_entries, flags,
                          [&](WeightSource& src) { return unet_create_impl(ctx, cfg, dtype, src, out); });
}
void sdxl_unet_destroy(sdxl_unet* u) {
  if (!u) return;
  if (u->owned) delete u->u;
  delete u;
}
int sdxl_unet_forward(sdxl_unet* u, void* stream, const float* x, const int32_t* timesteps, const float* context,
                      const float* label, int B, int H, int W, int n_ctx, float* out) {
  API_BEGIN
  SDXL_REQUIRE(u && x && timesteps && context && label && out, "null argument");
  use(u->ctx);
  u->u->forward_nchw(x, timesteps, context, n_ctx, label, B, H, W, out, pick(u->ctx, stream));
  API_END
}
int sdxl_unet_skip_count(const sdxl_unet_config* cfg) {
  try {
    std::vector<BlockDesc> inp, out; BlockDesc mid;
    unet_block_plan(to_cfg(cfg), inp, mid, out);
    return (int)inp.size() + 1;
  } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int sdxl_unet_skip_shape(const sdxl_unet_config* cfg, int index, int H, int W, int64_t chw[3]) {
  API_BEGIN
  if (!cfg || !chw) throw InvalidArgumentError("skip shape: null argument");
  const std::vector<UNet::SkipShape> sh = UNet::skip_shapes(to_cfg(cfg), H, W);
  if (index < 0 || index >= (int)sh.size()) throw InvalidArgumentError("skip shape: index outside 0 .. sdxl_unet_skip_count - 1");
  chw[0] = sh[index].C; chw[1] = sh[index].h; chw[2] = sh[index].w;
  API_END
}
int sdxl_unet_forward_residuals(sdxl_unet* u, void* stream, const float* x, const int32_t* timesteps, const float* context, const float* label,
                                int B, int H, int W, int n_ctx, const float* residuals, float scale, float* out) {
  API_BEGIN
  SDXL_REQUIRE(u && x && timesteps && context && label && out, "null argument");
  use(u->ctx);
  u->u->forward_residuals_nchw(x, timesteps, context, n_ctx, label, B, H, W, residuals, scale, out, pick(u->ctx, stream));
  API_END
}
int sdxl_unet_block(sdxl_unet* u, void* stream, int section, int index, const float* x, const float* emb, const float* context, int B, int c_in, int h,
                    int w, int n_ctx, float* out, int64_t out_shape[4]) {
  API_BEGIN
  if (!u) throw InvalidArgumentError("unet block: null handle");
  use(u->ctx);
  u->u->run_block(section, index, x, emb, context, n_ctx, B, c_in, h, w, out, out_shape, pick(u->ctx, stream));
  API_END
}
int sdxl_unet_set_graph(sdxl_unet* u, int enabled) {
  API_BEGIN
  SDXL_REQUIRE(u != nullptr, "null argument");
  u->u->set_use_graph(enabled != 0);
  API_END
}
int sdxl_unet_set_split_cfg(sdxl_unet* u, int enabled, int release_offset) {
  API_BEGIN
  SDXL_REQUIRE(u != nullptr && release_offset >= 0, "bad argument");
  u->u->set_split_cfg(enabled != 0, release_offset);
  API_END
}
int sdxl_unet_set_fused_cross_attention(sdxl_unet* u, int enabled) {
  API_BEGIN
  SDXL_REQUIRE(u != nullptr, "bad argument");
  u->u->set_fused_cross_attention(enabled != 0);
  API_END
}
int sdxl_unet_set_gn_from_producer(sdxl_unet* u, int enabled) {
  API_BEGIN
  SDXL_REQUIRE(u != nullptr, "bad argument");
  u->u->set_gn_from_producer(enabled != 0);
  API_END
}
int sdxl_unet_mix_classes(sdxl_unet* u, int* classes_out) {
  API_BEGIN
  SDXL_REQUIRE(u != nullptr && classes_out != nullptr, "null argument");
  *classes_out = u->u->mix_classes();
  API_END
}
int sdxl_unet_weight_arena(sdxl_unet* u, void** base, size_t* bytes) {
  API_BEGIN
  SDXL_REQUIRE(u && base && bytes, "null argument");
  *base = u->u->weight_base(); *bytes = u->u->weight_bytes();
  API_END
}

// ---------------------------------------------------------------------------------------------- Embedder (CLIP text encoders)
void sdxl_clip_config_clip_l(sdxl_clip_config* c) { if (c) *c = sdxl_clip_config{49408, 768, 768, 12, 77, 12, 1}; }
void sdxl_clip_config_open_clip_bigg(sdxl_clip_config* c) { if (c) *c = sdxl_clip_config{49408, 1280, 1280, 20, 77, 32, 0}; }
int sdxl_clip_param_count(const sdxl_clip_config* cfg) {
  try { return (int)clip_param_specs(to_ccfg(cfg)).size(); } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int sdxl_clip_param_spec(const sdxl_clip_config* cfg, int index, const char** name, int* ndim, int64_t shape[4], int* kind,
                         float* sc, float* mean) {
  API_BEGIN
  static thread_local std::vector<ParamSpec> cache; static thread_local sdxl_clip_config key;
  if (cache.empty() || std::memcmp(&key, cfg, sizeof(key)) != 0) { cache = clip_param_specs(to_ccfg(cfg)); key = *cfg; }
  return spec_out(cache, index, name, ndim, shape, kind, sc, mean);
  API_END
}
static int clip_create_impl(sdxl_ctx* ctx, const sdxl_clip_config* cfg, int dtype, WeightSource& src, sdxl_clip** out) {
  SDXL_REQUIRE(ctx && out, "bad argument");
  use(ctx);
  int cdt, sdt; no_mix(dtype); dtypes(dtype, cdt, sdt); no_split(cdt, "the CLIP text encoders");
  create_handle(ctx, out, [&](sdxl_clip& h) { h.c = new ClipText(to_ccfg(cfg), cdt, sdt, src, ctx->stream); });
  return SDXL_OK;
}
int sdxl_clip_create(sdxl_ctx* ctx, const sdxl_clip_config* cfg, int dtype, const float* weights_flat, sdxl_clip** out) {
  API_BEGIN
  SDXL_REQUIRE(weights_flat != nullptr, "null weights");
  const std::vector<ParamSpec> specs = clip_param_specs(to_ccfg(cfg));
  FlatSource src(weights_flat, specs);
  return clip_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
int sdxl_clip_create_f16(sdxl_ctx* ctx, const sdxl_clip_config* cfg, int dtype, const uint16_t* weights_flat_f16, sdxl_clip** out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && weights_flat_f16 != nullptr, "null argument");
  use(ctx);
  const std::vector<ParamSpec> specs = clip_param_specs(to_ccfg(cfg));
  FlatSourceF16 src(weights_flat_f16, specs);
  return clip_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
int sdxl_clip_create_synthetic(sdxl_ctx* ctx, const sdxl_clip_config* cfg, int dtype, uint64_t seed, sdxl_clip** out) {
  API_BEGIN
  SyntheticSource src(seed);
  return clip_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
void sdxl_clip_destroy(sdxl_clip* c) {
  if (!c) return;
  delete c->c;
  delete c;
}
int sdxl_clip_forward_hidden(sdxl_clip* c, void* stream, const int32_t* tokens, int n, int seq, int hidden_idx, float* out) {
  API_BEGIN
  SDXL_REQUIRE(c && tokens && out, "null argument");
  use(c->ctx);
  c->c->forward_hidden(tokens, n, seq, hidden_idx, out, pick(c->ctx, stream));
  API_END
}
int sdxl_clip_forward_hidden_pooled(sdxl_clip* c, void* stream, const int32_t* tokens, int n, int seq, int hidden_idx,
                                    float* out_hidden, float* out_pooled) {
  API_BEGIN
  SDXL_REQUIRE(c && tokens && out_hidden && out_pooled, "null argument");
  use(c->ctx);
  c->c->forward_hidden_pooled(tokens, n, seq, hidden_idx, out_hidden, out_pooled, pick(c->ctx, stream));
  API_END
}
int sdxl_conditioning_embedding(sdxl_ctx* ctx, void* stream, const float* pooled, int n, int E, const int32_t* values, int w,
                                int dim, float* out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && pooled && values && out && n > 0 && E > 0 && w > 0 && dim > 0 && dim % 2 == 0, "bad argument");
  use(ctx);
  launch_conditioning_embedding(pooled, E, values, w, dim, out, n, pick(ctx, stream));
  API_END
}
int sdxl_clip_weight_arena(sdxl_clip* c, void** base, size_t* bytes) {
  API_BEGIN
  SDXL_REQUIRE(c && base && bytes, "null argument");
  *base = c->c->weight_base(); *bytes = c->c->weight_bytes();
  API_END
}

// ---------------------------------------------------------------------------------------------- Diffuser
static int diffuser_create_impl(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, WeightSource& src, const float* alphas,
                                int n_train, sdxl_diffuser** out) {
  SDXL_REQUIRE(ctx && out && alphas && n_train > 0, "bad argument");
  use(ctx);
  int cdt, sdt; dtypes(dtype, cdt, sdt);
  create_handle(ctx, out, [&](sdxl_diffuser& h) {
    h.d = new Diffuser(to_cfg(cfg), cdt, sdt, src, alphas, n_train, ctx->stream, mix_of(dtype));
    h.view.ctx = ctx; h.view.u = &h.d->unet(); h.view.owned = false;
  });
  return SDXL_OK;
}
int sdxl_diffuser_create(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat, const float* alphas,
                         int n_train, sdxl_diffuser** out) {
  API_BEGIN
  SDXL_REQUIRE(weights_flat != nullptr, "null weights");
  const std::vector<ParamSpec> specs = unet_param_specs(to_cfg(cfg));
  FlatSource src(weights_flat, specs);
  return diffuser_create_impl(ctx, cfg, dtype, src, alphas, n_train, out);
  API_END
}
int sdxl_diffuser_create_f16(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const uint16_t* weights_flat_f16,
                             const float* alphas, int n_train, sdxl_diffuser** out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && weights_flat_f16 != nullptr, "null argument");
  use(ctx);
  const std::vector<ParamSpec> specs = unet_param_specs(to_cfg(cfg));
  FlatSourceF16 src(weights_flat_f16, specs);
  return diffuser_create_impl(ctx, cfg, dtype, src, alphas, n_train, out);
  API_END
}
int sdxl_diffuser_create_synthetic(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, uint64_t seed, const float* alphas,
                                   int n_train, sdxl_diffuser** out) {
  API_BEGIN
  SyntheticSource src(seed);
  return diffuser_create_impl(ctx, cfg, dtype, src, alphas, n_train, out);
  API_END
}
int sdxl_diffuser_create_lora(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat, const uint16_t* weights_flat_f16,
                              uint64_t synthetic_seed, const sdxl_lora_entry* entries, int n_entries, int flags, const float* alphas, int n_train,
                              sdxl_diffuser** out) {
  return create_with_lora(ctx, cfg, weights_flat, weights_flat_f16, synthetic_seed, entries, n_entries, flags,
                          [&](WeightSource& src) { return diffuser_create_impl(ctx, cfg, dtype, src, alphas, n_train, out); });
}
int sdxl_diffuser_create_empty(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* alphas, int n_train,
                               sdxl_diffuser** out) {
  API_BEGIN
  NullSource src;
  return diffuser_create_impl(ctx, cfg, dtype, src, alphas, n_train, out);
  API_END
}
int sdxl_vae_create_empty(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, int with_encoder, sdxl_vae** out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && out, "bad argument");
  use(ctx);
  int cdt, sdt; no_mix(dtype); dtypes(dtype, cdt, sdt);
  NullSource src;
  vae_create_impl(ctx, to_vcfg(cfg), cdt, &src, with_encoder ? &src : nullptr, out);
  API_END
}
int sdxl_unet_profile(sdxl_unet* u, void* stream, int B, int H, int W, float class_ms[5], int class_launches[5],
                      double class_flops[5]) {
  API_BEGIN
  SDXL_REQUIRE(u && class_ms && class_launches && class_flops, "null argument");
  use(u->ctx);
  u->u->profile(B, H, W, class_ms, class_launches, class_flops, pick(u->ctx, stream));
  API_END
}
int sdxl_unet_eager_forward_ms(sdxl_unet* u, void* stream, int B, int H, int W, float* ms_out) {
  API_BEGIN
  SDXL_REQUIRE(u && ms_out, "null argument");
  use(u->ctx);
  *ms_out = u->u->eager_ms(B, H, W, pick(u->ctx, stream));
  API_END
}
void sdxl_diffuser_destroy(sdxl_diffuser* d) {
  if (!d) return;
  delete d->d;
  delete d;
}
sdxl_unet* sdxl_diffuser_unet(sdxl_diffuser* d) { return d ? &d->view : nullptr; }

// per-entry guidance scales are one per batch entry of the call: refused before anything is launched
static const char* guidance_call_error(const sdxl_diffuser* d, const sdxl_conditioning* c) {
  if (!d || !c) return nullptr;     // reported by the call itself
  const Guidance& g = d->d->guidance();
  if (g.n_scales != 0 && g.n_scales != c->n) return "guidance: n_scales differs from the batch (cond.n)";
  return nullptr;
}
static Conditioning to_cond(const sdxl_conditioning* c) {
  SDXL_REQUIRE(c != nullptr, "null conditioning");
  Conditioning o;
  o.unconditional_context_full = c->unconditional_context_full;
  o.unconditional_context_open_clip = c->unconditional_context_open_clip;
  o.context_full = c->context_full; o.context_open_clip = c->context_open_clip;
  o.unconditional_channel_context = c->unconditional_channel_context;
  o.unconditional_channel_context_refiner = c->unconditional_channel_context_refiner;
  o.channel_context = c->channel_context; o.channel_context_refiner = c->channel_context_refiner;
  o.n = c->n; o.n_ctx = c->n_ctx; o.height = c->height; o.width = c->width;
  SDXL_REQUIRE(o.n >= 1 && o.n_ctx >= 1 && o.height >= 8 && o.width >= 8 && o.height % 8 == 0 && o.width % 8 == 0,
               "bad conditioning shape");
  return o;
}
int sdxl_sample_latent(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond, double cfg, int n_steps,
                       const float* noise0, float* out) {
  if (const char* m = guidance_call_error(d, cond)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  SDXL_REQUIRE(d && noise0 && out, "null argument");
  use(d->ctx);
  d->d->sample_latent(to_cond(cond), cfg, n_steps, noise0, out, pick(d->ctx, stream));
  API_END
}
int sdxl_sample_latent_with_inpainting(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond, double cfg, int n_steps,
                                       const float* reference, const uint8_t* mask, const float* noise0,
                                       const float* step_noise, float* out) {
  if (const char* m = guidance_call_error(d, cond)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  SDXL_REQUIRE(d && noise0 && out, "null argument");
  use(d->ctx);
  d->d->sample_latent_inpaint(to_cond(cond), cfg, n_steps, reference, mask, noise0, step_noise, out, pick(d->ctx, stream));
  API_END
}
int sdxl_refine_latent(sdxl_diffuser* d, void* stream, const float* latent, const sdxl_conditioning* cond, double cfg,
                       int step_start, int n_steps, const float* noise, float* out) {
  if (const char* m = guidance_call_error(d, cond)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  SDXL_REQUIRE(d && latent && noise && out, "null argument");
  use(d->ctx);
  d->d->refine_latent(latent, to_cond(cond), cfg, step_start, n_steps, noise, out, pick(d->ctx, stream));
  API_END
}
// seeded forms: argument errors are SDXL_ERR_INVALID (nothing was launched, the handle is untouched)
static const char* seeded_args_error(const uint64_t* seeds, double eta) {
  if (!seeds) return "seeds is NULL: one 64-bit seed per batch entry";
  if (!(eta >= 0.0 && eta <= 1.0)) return "eta must be a finite value in [0, 1]";
  return nullptr;
}
int sdxl_gen_noise(sdxl_ctx* ctx, void* stream, const uint64_t* seeds, uint32_t draw, int n, int h, int w, float* out) {
  if (!ctx || !out) return fail(SDXL_ERR_INVALID, "null argument");
  if (!seeds) return fail(SDXL_ERR_INVALID, "seeds is NULL: one 64-bit seed per batch entry");
  if (n < 1 || h < 1 || w < 1 || (int64_t)h * w > (int64_t)1 << 30) return fail(SDXL_ERR_INVALID, "gen_noise: n, h, w out of range");
  API_BEGIN
  use(ctx);
  launch_seeded_noise(out, seeds, draw, n, h * w, pick(ctx, stream));
  API_END
}
int sdxl_sample_latent_seeded(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond, double cfg, int n_steps,
                              const uint64_t* seeds, double eta, float* out) {
  if (const char* m = seeded_args_error(seeds, eta)) return fail(SDXL_ERR_INVALID, m);
  if (const char* m = guidance_call_error(d, cond)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  SDXL_REQUIRE(d && out, "null argument");
  use(d->ctx);
  d->d->sample_latent_seeded(to_cond(cond), cfg, n_steps, seeds, eta, out, pick(d->ctx, stream));
  API_END
}
int sdxl_sample_latent_with_inpainting_seeded(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond, double cfg, int n_steps,
                                              const float* reference, const uint8_t* mask, const uint64_t* seeds, double eta,
                                              float* out) {
  if (const char* m = seeded_args_error(seeds, eta)) return fail(SDXL_ERR_INVALID, m);
  if (const char* m = guidance_call_error(d, cond)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  SDXL_REQUIRE(d && out, "null argument");
  use(d->ctx);
  d->d->sample_latent_inpaint_seeded(to_cond(cond), cfg, n_steps, reference, mask, seeds, eta, out, pick(d->ctx, stream));
  API_END
}
int sdxl_refine_latent_seeded(sdxl_diffuser* d, void* stream, const float* latent, const sdxl_conditioning* cond, double cfg,
                              int step_start, int n_steps, const uint64_t* seeds, double eta, float* out) {
  if (const char* m = seeded_args_error(seeds, eta)) return fail(SDXL_ERR_INVALID, m);
  if (const char* m = guidance_call_error(d, cond)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  SDXL_REQUIRE(d && latent && out, "null argument");
  use(d->ctx);
  d->d->refine_latent_seeded(latent, to_cond(cond), cfg, step_start, n_steps, seeds, eta, out, pick(d->ctx, stream));
  API_END
}
int sdxl_continue_latent(sdxl_diffuser* d, void* stream, const float* latent, const sdxl_conditioning* cond, double cfg, int n_steps,
                         const float* noise, const uint64_t* seeds, double eta, int renoise, float* out) {
  if (!(eta >= 0.0 && eta <= 1.0)) return fail(SDXL_ERR_INVALID, "eta must be a finite value in [0, 1]");
  if (const char* m = guidance_call_error(d, cond)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  if (!d || !latent || !out) throw InvalidArgumentError("null argument");
  use(d->ctx);
  d->d->continue_latent(latent, to_cond(cond), cfg, n_steps, noise, seeds, eta, renoise != 0, out, pick(d->ctx, stream));
  API_END
}
int sdxl_step_count(int n_steps, int step_start, int n_train) {
  try { return (int)Diffuser::step_schedule(n_steps, step_start, n_train).size(); }
  catch (const std::exception& e) { g_err = e.what(); return -1; }
}
static bool known_solver(int solver) {
  return solver == SDXL_SOLVER_DDIM || solver == SDXL_SOLVER_DPMPP_2M || solver == SDXL_SOLVER_LCM || solver == SDXL_SOLVER_TCD ||
         solver == SDXL_SOLVER_DPMPP_3M;
}
static const char* const kUnknownSolver =
    "unknown solver (SDXL_SOLVER_DDIM, SDXL_SOLVER_DPMPP_2M, SDXL_SOLVER_DPMPP_3M, SDXL_SOLVER_LCM, SDXL_SOLVER_TCD)";
// the entries with four-column rows and one history output cannot carry the 3M solver's c_2 and second history
static const char* const kSolver3MEntry =
    "solver DPMPP_3M has five-column rows and two histories: use sdxl_solver_rows / sdxl_sampler_step_replay_levels";
// solver: a per-handle option; an unknown value is an argument error and leaves the handle as it was
int sdxl_diffuser_set_solver(sdxl_diffuser* d, int solver) {
  if (!d) return fail(SDXL_ERR_INVALID, "null argument");
  if (!known_solver(solver)) return fail(SDXL_ERR_INVALID, kUnknownSolver);
  API_BEGIN
  d->d->set_solver(solver);
  API_END
}
int sdxl_diffuser_get_solver(sdxl_diffuser* d, int* solver_out) {
  if (!d || !solver_out) return fail(SDXL_ERR_INVALID, "null argument");
  *solver_out = d->d->solver();
  return SDXL_OK;
}
// timestep list: a per-handle option; a list the check refuses is an argument error and leaves the handle as it was
int sdxl_diffuser_set_timesteps(sdxl_diffuser* d, const int32_t* timesteps, int n) { return sdxl_diffuser_set_timesteps_end(d, timesteps, n, -1); }
int sdxl_diffuser_set_timesteps_end(sdxl_diffuser* d, const int32_t* timesteps, int n, int t_end) {
  if (!d) return fail(SDXL_ERR_INVALID, "null argument");
  static_assert(sizeof(int32_t) == sizeof(int), "lists travel as int");
  API_BEGIN
  if (timesteps && n < 0) throw InvalidArgumentError("timesteps: the list needs 1..n_train_steps entries");
  d->d->set_timesteps((const int*)timesteps, n, t_end);
  API_END
}
int sdxl_diffuser_get_timesteps_end(sdxl_diffuser* d, int* t_end_out) {
  if (!d || !t_end_out) return fail(SDXL_ERR_INVALID, "null argument");
  *t_end_out = d->d->timesteps().empty() ? -1 : d->d->timesteps_end();
  return SDXL_OK;
}
// sigma list: a per-handle option like the timestep list; a list the check refuses is an argument error and leaves the handle as it was
int sdxl_diffuser_set_sigmas(sdxl_diffuser* d, const double* sigmas, int n, double sigma_end, int flags) {
  if (!d) return fail(SDXL_ERR_INVALID, "null argument");
  API_BEGIN
  if (sigmas && n < 0) throw InvalidArgumentError("sigmas: the list needs 1..n_train_steps entries");
  d->d->set_sigmas(sigmas, n, sigma_end, flags);
  API_END
}
int sdxl_diffuser_get_sigmas(sdxl_diffuser* d, double* out, int capacity, double* sigma_end_out, int* flags_out) {
  if (!d) return fail(SDXL_ERR_INVALID, "null argument");
  const std::vector<double>& sg = d->d->sigmas();
  if (sg.empty()) return 0;
  if (!out || capacity < (int)sg.size()) return fail(SDXL_ERR_INVALID, "sigmas: capacity is smaller than the handle's list");
  std::copy(sg.begin(), sg.end(), out);
  if (sigma_end_out) *sigma_end_out = d->d->sigma_end();
  if (flags_out) *flags_out = d->d->sigma_flags();
  return (int)sg.size();
}
static const char* table_error(const float* alphas_cumprod_host, int n_train_steps) {      // a table a sigma entry can read
  if (!alphas_cumprod_host) return "null argument";
  if (n_train_steps < 2) return "sigmas: the alphas_cumprod table needs at least two entries";
  for (int i = 0; i < n_train_steps; ++i)
    if (!(alphas_cumprod_host[i] >= 0.f && alphas_cumprod_host[i] < 1.f)) return "alphas_cumprod outside (0, 1)";
  return nullptr;
}
int sdxl_sigma_to_timestep(const float* alphas_cumprod_host, int n_train_steps, double sigma, int flags, double* t_out) {
  if (!t_out) return fail(SDXL_ERR_INVALID, "null argument");
  if (const char* m = table_error(alphas_cumprod_host, n_train_steps)) return fail(SDXL_ERR_INVALID, m);
  if (const char* m = Diffuser::sigmas_error(&sigma, 1, 0.0, flags, n_train_steps)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  const std::vector<double> alphas(alphas_cumprod_host, alphas_cumprod_host + n_train_steps);
  *t_out = Diffuser::sigma_to_t(alphas.data(), n_train_steps, sigma, flags);
  API_END
}
// host logic only: the published sigma spacings
int sdxl_sigma_schedule(int kind, int n_steps, const float* alphas_cumprod_host, int n_train_steps, double sigma_min, double sigma_max, double rho,
                        double* out, int capacity) {
  if (!out) return fail(SDXL_ERR_INVALID, "null argument");
  if (const char* m = table_error(alphas_cumprod_host, n_train_steps)) return fail(SDXL_ERR_INVALID, m);
  if (n_steps < 1 || n_steps > n_train_steps) return fail(SDXL_ERR_INVALID, "n_steps out of range (1..n_train_steps)");
  const auto sigma_of = [&](int j) { const double a = (double)alphas_cumprod_host[j]; return std::sqrt((1.0 - a) / a); };
  std::vector<double> sg;
  if (kind == SDXL_SIGMAS_OF_TIMESTEPS) {
    for (int t : Diffuser::step_schedule(n_steps, 0, n_train_steps)) sg.push_back(sigma_of(t));
  } else if (kind == SDXL_SIGMAS_KARRAS || kind == SDXL_SIGMAS_EXPONENTIAL) {
    const double lo = sigma_min > 0.0 ? sigma_min : sigma_of(0), hi = sigma_max > 0.0 ? sigma_max : sigma_of(n_train_steps - 1);
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo > 0.0 && lo < hi)) return fail(SDXL_ERR_INVALID, "sigmas: needs finite 0 < sigma_min < sigma_max");
    if (kind == SDXL_SIGMAS_KARRAS && !(std::isfinite(rho) && rho > 0.0)) return fail(SDXL_ERR_INVALID, "sigmas: rho must be finite and > 0 (Karras et al. use 7)");
    for (int i = 0; i < n_steps; ++i) {
      const double ramp = n_steps == 1 ? 0.0 : (double)i / (double)(n_steps - 1);
      if (kind == SDXL_SIGMAS_KARRAS) {
        const double hi_r = std::pow(hi, 1.0 / rho), lo_r = std::pow(lo, 1.0 / rho);
        sg.push_back(std::pow(hi_r + ramp * (lo_r - hi_r), rho));
      } else {
        const double lh = std::log(hi), ll = std::log(lo);
        sg.push_back(std::exp(lh + ramp * (ll - lh)));
      }
    }
  } else {
    return fail(SDXL_ERR_INVALID, "sigmas: unknown kind (SDXL_SIGMAS_KARRAS, _EXPONENTIAL, _OF_TIMESTEPS)");
  }
  for (double v : sg)
    if (!(std::isfinite(v) && v > 0.0)) return fail(SDXL_ERR_INVALID, "sigmas: the table gives a sigma that is not finite and > 0 (alphas_cumprod == 0 at a timestep)");
  if (capacity < (int)sg.size()) return fail(SDXL_ERR_INVALID, "sigmas: capacity is smaller than the list");
  std::copy(sg.begin(), sg.end(), out);
  return (int)sg.size();
}
int sdxl_diffuser_get_timesteps(sdxl_diffuser* d, int32_t* out, int capacity) {
  if (!d) return fail(SDXL_ERR_INVALID, "null argument");
  const std::vector<int>& ts = d->d->timesteps();
  if (ts.empty()) return 0;
  if (!out || capacity < (int)ts.size()) return fail(SDXL_ERR_INVALID, "timesteps: capacity is smaller than the handle's list");
  std::copy(ts.begin(), ts.end(), out);
  return (int)ts.size();
}
// host logic only: the published spacings as lists (integer arithmetic but for the one rint of SDXL_SCHEDULE_TRAILING)
int sdxl_timestep_schedule(int kind, int n_steps, int n_train_steps, int param, int32_t* out, int capacity) {
  if (!out) return fail(SDXL_ERR_INVALID, "null argument");
  if (n_train_steps < 1 || n_steps < 1 || n_steps > n_train_steps) return fail(SDXL_ERR_INVALID, "n_steps out of range (1..n_train_steps)");
  std::vector<int> ts;
  switch (kind) {
    case SDXL_SCHEDULE_REFERENCE:
      ts = Diffuser::step_schedule(n_steps, 0, n_train_steps);
      break;
    case SDXL_SCHEDULE_TRAILING: {
      const double step = (double)n_train_steps / (double)n_steps;
      for (int i = 0; i < n_steps; ++i) ts.push_back((int)std::nearbyint((double)n_train_steps - (double)i * step) - 1);     // ties to even
      break;
    }
    case SDXL_SCHEDULE_LEADING: {
      const int step = n_train_steps / n_steps;
      if (param < 0 || (int64_t)(n_steps - 1) * step + param >= n_train_steps)
        return fail(SDXL_ERR_INVALID, "timestep_schedule: the offset puts the first timestep outside 0..n_train_steps-1");
      for (int i = 0; i < n_steps; ++i) ts.push_back((n_steps - 1 - i) * step + param);
      break;
    }
    case SDXL_SCHEDULE_LCM: {
      const int O = param;
      if (O < 1 || O > n_train_steps) return fail(SDXL_ERR_INVALID, "timestep_schedule: origin steps out of range (1..n_train_steps)");
      if (n_steps > O) return fail(SDXL_ERR_INVALID, "timestep_schedule: n_steps exceeds the origin steps");
      const int k = n_train_steps / O;
      for (int i = 0; i < n_steps; ++i) ts.push_back((O - (int)((int64_t)i * O / n_steps)) * k - 1);
      break;
    }
    default:
      return fail(SDXL_ERR_INVALID, "timestep_schedule: unknown kind (SDXL_SCHEDULE_REFERENCE, _TRAILING, _LEADING, _LCM)");
  }
  if (capacity < (int)ts.size()) return fail(SDXL_ERR_INVALID, "timestep_schedule: capacity is smaller than the list");
  std::copy(ts.begin(), ts.end(), out);
  return (int)ts.size();
}
// host logic of the sampler's coefficient table -- no device needed; the function Diffuser::diffuse fills its row tables from.
// The checks of a table call in their order: the scalars, then (where there is no list) the reference rule's two numbers
static const char* solver_args_error(const float* alphas_cumprod_host, int n_train_steps, int solver, double eta) {
  if (!alphas_cumprod_host) return "null argument";
  if (!known_solver(solver)) return kUnknownSolver;
  if (!(eta >= 0.0 && eta <= 1.0)) return "eta must be a finite value in [0, 1]";
  return nullptr;
}
static const char* schedule_args_error(const float* alphas_cumprod_host, int n_train_steps, int n_steps, int step_start, int solver, double eta) {
  if (const char* m = solver_args_error(alphas_cumprod_host, n_train_steps, solver, eta)) return m;
  if (n_train_steps < 1 || n_steps < 1 || n_steps > n_train_steps) return "n_steps out of range (1..n_train_steps)";
  if (step_start < 0 || step_start >= n_train_steps) return "step_start out of range (0..n_train_steps-1)";
  return nullptr;
}
static const char* list_args_error(const float* alphas_cumprod_host, int n_train_steps, const int32_t* timesteps, int n, int solver, double eta,
                                   int t_end = -1) {
  if (const char* m = solver_args_error(alphas_cumprod_host, n_train_steps, solver, eta)) return m;
  if (n_train_steps < 1) return "n_train_steps out of range";
  if (const char* m = Diffuser::timesteps_end_error((const int*)timesteps, n, t_end, n_train_steps)) return m;
  if (solver == SDXL_SOLVER_LCM && eta != 0.0) return "solver LCM takes no eta: eta must be 0 (SDXL_SOLVER_LCM)";
  return nullptr;
}
static const char* alphas_error(const float* alphas_cumprod_host, int n_train_steps) {
  for (int i = 0; i < n_train_steps; ++i)
    if (!(alphas_cumprod_host[i] > 0.f && alphas_cumprod_host[i] < 1.f)) return "alphas_cumprod outside (0, 1)";
  return nullptr;
}
// the table under a prediction type (a valid list): SDXL_PREDICTION_V admits 0 in it, and the schedule decides where it may stand;
// under SDXL_PREDICTION_EPSILON a 0 at a sampled timestep gets the message that names the remedy, any other value outside (0, 1) the old one
// ts: a list Diffuser::timesteps_end_error accepts
static const char* alphas_error_pred(const float* alphas_cumprod_host, int n_train_steps, const std::vector<int>& ts, int prediction, int t_end = -1) {
  if (prediction != SDXL_PREDICTION_EPSILON && prediction != SDXL_PREDICTION_V) return "unknown prediction (SDXL_PREDICTION_EPSILON, SDXL_PREDICTION_V)";
  for (int i = 0; i < n_train_steps; ++i)
    if (!(alphas_cumprod_host[i] >= 0.f && alphas_cumprod_host[i] < 1.f)) return "alphas_cumprod outside (0, 1)";
  const std::vector<double> alphas(alphas_cumprod_host, alphas_cumprod_host + n_train_steps);
  const Schedule sc = Diffuser::schedule_of_timesteps(alphas.data(), n_train_steps, ts.data(), (int)ts.size(), t_end);
  if (const char* m = Diffuser::schedule_error(sc, prediction)) return m;
  return prediction == SDXL_PREDICTION_EPSILON ? alphas_error(alphas_cumprod_host, n_train_steps) : nullptr;
}
// the schedule a sdxl_schedule_desc describes, with every check of the list entries: nullptr and (alphas, sc) filled, or the complaint
static const char* desc_schedule(const sdxl_schedule_desc* k, int solver, double eta, int prediction, std::vector<double>& alphas, Schedule& sc) {
  if (!k) return "null argument";
  if ((k->timesteps != nullptr) == (k->sigmas != nullptr)) return "schedule: give exactly one of timesteps and sigmas";
  if (k->timesteps) {
    if (const char* m = list_args_error(k->alphas_cumprod_host, k->n_train_steps, k->timesteps, k->n, solver, eta, k->t_end)) return m;
    const std::vector<int> ts(k->timesteps, k->timesteps + k->n);
    if (const char* m = alphas_error_pred(k->alphas_cumprod_host, k->n_train_steps, ts, prediction, k->t_end)) return m;
    alphas.assign(k->alphas_cumprod_host, k->alphas_cumprod_host + k->n_train_steps);
    sc = Diffuser::schedule_of_timesteps(alphas.data(), k->n_train_steps, ts.data(), k->n, k->t_end);
    return nullptr;
  }
  if (const char* m = solver_args_error(k->alphas_cumprod_host, k->n_train_steps, solver, eta)) return m;
  if (const char* m = table_error(k->alphas_cumprod_host, k->n_train_steps)) return m;
  if (const char* m = Diffuser::sigmas_error(k->sigmas, k->n, k->sigma_end, k->flags, k->n_train_steps)) return m;
  if (solver == SDXL_SOLVER_LCM && eta != 0.0) return "solver LCM takes no eta: eta must be 0 (SDXL_SOLVER_LCM)";
  if (solver == SDXL_SOLVER_TCD)
    return "solver TCD reads alphas_cumprod at floor((1 - gamma) t'), a training timestep: it does not run on sigmas (use a timestep list)";
  if (prediction != SDXL_PREDICTION_EPSILON && prediction != SDXL_PREDICTION_V) return "unknown prediction (SDXL_PREDICTION_EPSILON, SDXL_PREDICTION_V)";
  alphas.assign(k->alphas_cumprod_host, k->alphas_cumprod_host + k->n_train_steps);
  sc = Diffuser::schedule_of_sigmas(alphas.data(), k->n_train_steps, k->sigmas, k->n, k->sigma_end, k->flags);
  return Diffuser::schedule_error(sc, prediction);
}
int sdxl_solver_rows(const sdxl_schedule_desc* schedule, int solver, int prediction, double eta, double* out, int capacity_rows) {
  if (!out) return fail(SDXL_ERR_INVALID, "null argument");
  std::vector<double> alphas;
  Schedule sc;
  if (const char* m = desc_schedule(schedule, solver, eta, prediction, alphas, sc)) return fail(SDXL_ERR_INVALID, m);
  if (capacity_rows < (int)sc.size()) return fail(SDXL_ERR_INVALID, "capacity_rows is smaller than the list");
  API_BEGIN
  std::vector<double> rows((size_t)kRowCols * sc.size());
  Diffuser::solver_coefficients(alphas.data(), (int)alphas.size(), sc, solver, eta, rows.data(), prediction);
  std::copy(rows.begin(), rows.end(), out);
  API_END
}
int sdxl_solver_coefficients_ts(const float* alphas_cumprod_host, int n_train_steps, const int32_t* timesteps, int n, int solver, int prediction,
                                double eta, double* out, int capacity_steps) {
  if (!out) return fail(SDXL_ERR_INVALID, "null argument");
  if (solver == SDXL_SOLVER_DPMPP_3M && alphas_cumprod_host) return fail(SDXL_ERR_INVALID, kSolver3MEntry);
  if (const char* m = list_args_error(alphas_cumprod_host, n_train_steps, timesteps, n, solver, eta)) return fail(SDXL_ERR_INVALID, m);
  if (capacity_steps < n) return fail(SDXL_ERR_INVALID, "capacity_steps is smaller than the list (sdxl_step_count for the reference's rule)");
  const std::vector<int> ts(timesteps, timesteps + n);
  if (const char* m = alphas_error_pred(alphas_cumprod_host, n_train_steps, ts, prediction)) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  std::vector<double> alphas(alphas_cumprod_host, alphas_cumprod_host + n_train_steps);   // elem -> f64 as the Diffuser holds them
  const Schedule sc = Diffuser::schedule_of_timesteps(alphas.data(), n_train_steps, ts.data(), n);
  std::vector<double> rows((size_t)kRowCols * n);
  Diffuser::solver_coefficients(alphas.data(), n_train_steps, sc, solver, eta, rows.data(), prediction);
  for (int i = 0; i < n; ++i) {      // the four columns these entries have always had: c_2 is 0 for their solvers
    const double* r = &rows[(size_t)kRowCols * i];
    out[4 * i] = r[0]; out[4 * i + 1] = r[1]; out[4 * i + 2] = r[2]; out[4 * i + 3] = r[4];
  }
  API_END
}
int sdxl_solver_coefficients_pred(const float* alphas_cumprod_host, int n_train_steps, int n_steps, int step_start, int solver, int prediction,
                                  double eta, double* out, int capacity_steps) {
  if (!out) return fail(SDXL_ERR_INVALID, "null argument");
  if (solver == SDXL_SOLVER_DPMPP_3M && alphas_cumprod_host) return fail(SDXL_ERR_INVALID, kSolver3MEntry);
  if (const char* m = schedule_args_error(alphas_cumprod_host, n_train_steps, n_steps, step_start, solver, eta)) return fail(SDXL_ERR_INVALID, m);
  const std::vector<int> ts = Diffuser::step_schedule(n_steps, step_start, n_train_steps);     // the reference's rule as a list
  return sdxl_solver_coefficients_ts(alphas_cumprod_host, n_train_steps, ts.data(), (int)ts.size(), solver, prediction, eta, out, capacity_steps);
}
int sdxl_solver_coefficients(const float* alphas_cumprod_host, int n_train_steps, int n_steps, int step_start, int solver, double eta,
                             double* out, int capacity_steps) {
  return sdxl_solver_coefficients_pred(alphas_cumprod_host, n_train_steps, n_steps, step_start, solver, SDXL_PREDICTION_EPSILON, eta, out,
                                       capacity_steps);
}
// prediction: a per-handle option like the solver; an unknown value is an argument error and leaves the handle as it was
int sdxl_diffuser_set_prediction(sdxl_diffuser* d, int prediction) {
  if (!d) return fail(SDXL_ERR_INVALID, "null argument");
  if (prediction != SDXL_PREDICTION_EPSILON && prediction != SDXL_PREDICTION_V)
    return fail(SDXL_ERR_INVALID, "unknown prediction (SDXL_PREDICTION_EPSILON, SDXL_PREDICTION_V)");
  API_BEGIN
  d->d->set_prediction(prediction);
  API_END
}
int sdxl_diffuser_get_prediction(sdxl_diffuser* d, int* prediction_out) {
  if (!d || !prediction_out) return fail(SDXL_ERR_INVALID, "null argument");
  *prediction_out = d->d->prediction();
  return SDXL_OK;
}
// Lin et al. 2023, Algorithm 1 on s = sqrt(alphas_cumprod), f64: shift so that s[T-1] = 0, scale so that s[0] keeps its value
int sdxl_rescale_zero_terminal_snr(const float* alphas_cumprod_in, int n_train_steps, float* alphas_cumprod_out) {
  if (!alphas_cumprod_in || !alphas_cumprod_out) return fail(SDXL_ERR_INVALID, "null argument");
  if (n_train_steps < 2) return fail(SDXL_ERR_INVALID, "rescale_zero_terminal_snr: n_train_steps must be at least 2");
  for (int i = 0; i < n_train_steps; ++i) {
    if (!(alphas_cumprod_in[i] > 0.f && alphas_cumprod_in[i] < 1.f)) return fail(SDXL_ERR_INVALID, "alphas_cumprod outside (0, 1)");
    if (i > 0 && !(alphas_cumprod_in[i] < alphas_cumprod_in[i - 1])) return fail(SDXL_ERR_INVALID, "alphas_cumprod is not strictly decreasing");
  }
  const double s0 = std::sqrt((double)alphas_cumprod_in[0]), sT = std::sqrt((double)alphas_cumprod_in[n_train_steps - 1]);
  for (int i = 0; i < n_train_steps; ++i) {     // in == out allowed: entry i is read before it is written, s0 and sT are held
    const double s = (std::sqrt((double)alphas_cumprod_in[i]) - sT) * s0 / (s0 - sT);
    alphas_cumprod_out[i] = (float)(s * s);
  }
  return SDXL_OK;
}
// guidance: a per-handle option; options the check refuses are an argument error and leave the handle as it was
static Guidance to_guidance(const sdxl_guidance* g) {
  Guidance o;
  if (!g) return o;
  o.mode = g->mode; o.rescale = g->rescale; o.n_scales = g->n_scales; o.t_lo = g->t_lo; o.t_hi = g->t_hi;
  for (int b = 0; b < kMaxSeeds; ++b) o.scales[b] = g->scales[b];
  return o;
}
void sdxl_guidance_default(sdxl_guidance* g) {
  if (!g) return;
  const Guidance o;
  g->mode = o.mode; g->rescale = o.rescale; g->n_scales = o.n_scales; g->t_lo = o.t_lo; g->t_hi = o.t_hi;
  for (int b = 0; b < kMaxSeeds; ++b) g->scales[b] = o.scales[b];
}
int sdxl_guidance_check(const sdxl_guidance* g, int is_refiner) {
  if (!g) return fail(SDXL_ERR_INVALID, "null argument");
  if (const char* m = Diffuser::guidance_error(to_guidance(g), is_refiner != 0)) return fail(SDXL_ERR_INVALID, m);
  return SDXL_OK;
}
int sdxl_diffuser_set_guidance(sdxl_diffuser* d, const sdxl_guidance* g) {
  if (!d) return fail(SDXL_ERR_INVALID, "null argument");
  const Guidance o = to_guidance(g);
  if (const char* m = Diffuser::guidance_error(o, d->d->is_refiner())) return fail(SDXL_ERR_INVALID, m);
  API_BEGIN
  d->d->set_guidance(o);
  API_END
}
int sdxl_diffuser_get_guidance(sdxl_diffuser* d, sdxl_guidance* out) {
  if (!d || !out) return fail(SDXL_ERR_INVALID, "null argument");
  const Guidance& o = d->d->guidance();
  out->mode = o.mode; out->rescale = o.rescale; out->n_scales = o.n_scales; out->t_lo = o.t_lo; out->t_hi = o.t_hi;
  for (int b = 0; b < kMaxSeeds; ++b) out->scales[b] = o.scales[b];
  return SDXL_OK;
}
// ---------------------------------------------------------------------------------------------- ControlNet
static ControlCfg to_ccfg_control(const sdxl_controlnet_config* c) {
  SDXL_REQUIRE(c != nullptr, "null config");
  ControlCfg k;
  k.unet = to_cfg(&c->unet);
  k.hint_in = c->hint_in_channels;
  SDXL_REQUIRE(k.hint_in >= 1 && k.hint_in <= 64, "controlnet: hint_in_channels out of range (1..64)");
  for (int i = 0; i < 4; ++i) {
    k.hint_channels[i] = c->hint_channels[i];
    SDXL_REQUIRE(k.hint_channels[i] >= 8 && k.hint_channels[i] % 8 == 0 && k.hint_channels[i] <= 4096, "controlnet: hint_channels must be multiples of 8 in 8..4096");
  }
  return k;
}
static int controlnet_create_impl(sdxl_ctx* ctx, const sdxl_controlnet_config* cfg, int dtype, WeightSource& src, sdxl_controlnet** out) {
  if (!ctx || !out || !cfg) throw InvalidArgumentError("controlnet: null argument");
  if (dtype != SDXL_DTYPE_F32 && dtype != SDXL_DTYPE_F16 && dtype != SDXL_DTYPE_F32_SPLIT)
    throw InvalidArgumentError("controlnet: dtype " + std::to_string(dtype) + " is not supported: a control net takes SDXL_DTYPE_F32, SDXL_DTYPE_F16 or SDXL_DTYPE_F32_SPLIT");
  if (cfg->unet.is_refiner != 0) throw InvalidArgumentError("controlnet: there is no refiner ControlNet (unet.is_refiner != 0)");
  use(ctx);
  int cdt, sdt; dtypes(dtype, cdt, sdt);
  const ControlCfg cc = to_ccfg_control(cfg);
  create_handle(ctx, out, [&](sdxl_controlnet& h) { h.c = new UNet(cc, cdt, sdt, src, ctx->stream); });
  return SDXL_OK;
}
void sdxl_controlnet_config_default(const sdxl_unet_config* unet, sdxl_controlnet_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  if (unet) cfg->unet = *unet;
  cfg->hint_in_channels = 3;
  const int hc[4] = {16, 32, 96, 256};
  for (int i = 0; i < 4; ++i) cfg->hint_channels[i] = hc[i];
}
int sdxl_controlnet_param_count(const sdxl_controlnet_config* cfg) {
  try { return (int)controlnet_param_specs(to_ccfg_control(cfg)).size(); } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int sdxl_controlnet_param_spec(const sdxl_controlnet_config* cfg, int index, const char** name, int* ndim, int64_t shape[4], int* kind,
                               float* sc, float* mean) {
  API_BEGIN
  SDXL_REQUIRE(cfg != nullptr, "null config");
  static thread_local std::vector<ParamSpec> cache; static thread_local sdxl_controlnet_config key;
  if (cache.empty() || std::memcmp(&key, cfg, sizeof(key)) != 0) { cache = controlnet_param_specs(to_ccfg_control(cfg)); key = *cfg; }
  return spec_out(cache, index, name, ndim, shape, kind, sc, mean);
  API_END
}
int sdxl_controlnet_create(sdxl_ctx* ctx, const sdxl_controlnet_config* cfg, int dtype, const float* weights_flat, sdxl_controlnet** out) {
  API_BEGIN
  if (!weights_flat || !cfg) throw InvalidArgumentError("controlnet: null argument");
  const std::vector<ParamSpec> specs = controlnet_param_specs(to_ccfg_control(cfg));
  FlatSource src(weights_flat, specs);
  return controlnet_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
int sdxl_controlnet_create_f16(sdxl_ctx* ctx, const sdxl_controlnet_config* cfg, int dtype, const uint16_t* weights_flat_f16, sdxl_controlnet** out) {
  API_BEGIN
  if (!ctx || !weights_flat_f16 || !cfg) throw InvalidArgumentError("controlnet: null argument");
  use(ctx);
  const std::vector<ParamSpec> specs = controlnet_param_specs(to_ccfg_control(cfg));
  FlatSourceF16 src(weights_flat_f16, specs);
  return controlnet_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
int sdxl_controlnet_create_synthetic(sdxl_ctx* ctx, const sdxl_controlnet_config* cfg, int dtype, uint64_t seed, sdxl_controlnet** out) {
  API_BEGIN
  SyntheticSource src(seed);
  return controlnet_create_impl(ctx, cfg, dtype, src, out);
  API_END
}
void sdxl_controlnet_destroy(sdxl_controlnet* c) { delete c; }
int sdxl_controlnet_embed_hint(sdxl_controlnet* c, void* stream, const float* hint, int n, int H8, int W8, float* out) {
  API_BEGIN
  if (!c || !hint || !out) throw InvalidArgumentError("controlnet: null argument");
  if (n < 1 || n > 8 || H8 <= 0 || W8 <= 0 || H8 % 8 != 0 || W8 % 8 != 0) throw InvalidArgumentError("controlnet: n must be in 1..8 and the hint 8 x a valid latent size");
  use(c->ctx);
  c->c->embed_hint_nchw(hint, n, H8 / 8, W8 / 8, out, pick(c->ctx, stream));
  API_END
}
int sdxl_controlnet_forward(sdxl_controlnet* c, void* stream, const float* x, const int32_t* timesteps, const float* context, const float* label,
                            const float* hint, int B, int H, int W, int n_ctx, float* residuals_out) {
  API_BEGIN
  if (!c || !x || !timesteps || !context || !label || !hint || !residuals_out) throw InvalidArgumentError("controlnet: null argument");
  use(c->ctx);
  c->c->control_forward_nchw(x, timesteps, context, n_ctx, label, hint, B, H, W, residuals_out, pick(c->ctx, stream));
  API_END
}
// control options: host logic only
static Control to_control(const sdxl_control* c) {
  Control o;
  if (!c) return o;
  o.scale = c->scale; o.n_scales = c->n_scales; o.t_lo = c->t_lo; o.t_hi = c->t_hi; o.cond_only = c->cond_only != 0;
  for (int b = 0; b < kMaxSeeds; ++b) o.scales[b] = c->scales[b];
  return o;
}
void sdxl_control_default(sdxl_control* c) {
  if (!c) return;
  const Control o;
  c->scale = o.scale; c->n_scales = o.n_scales; c->t_lo = o.t_lo; c->t_hi = o.t_hi; c->cond_only = o.cond_only;
  for (int b = 0; b < kMaxSeeds; ++b) c->scales[b] = o.scales[b];
}
int sdxl_control_check(const sdxl_control* c, int single_branch) {
  if (!c) return fail(SDXL_ERR_INVALID, "null argument");
  if (const char* m = control_error(to_control(c), single_branch != 0)) return fail(SDXL_ERR_INVALID, m);
  return SDXL_OK;
}
int sdxl_control_scale_table(const sdxl_control* c, int n, int single_branch, const int32_t* timesteps, int iters, float* out) {
  if (!c) return fail(SDXL_ERR_INVALID, "null argument");
  if (const char* m = control_scale_table(to_control(c), n, single_branch != 0, timesteps, iters, out)) return fail(SDXL_ERR_INVALID, m);
  return SDXL_OK;
}
int sdxl_cfg_rescale_factors(sdxl_ctx* ctx, void* stream, const float* eps, int n, int HW, const float* scales, float rescale,
                             float* factors_out) {
  if (!ctx || !eps || !scales || !factors_out) return fail(SDXL_ERR_INVALID, "null argument");
  if (n < 1 || n > kMaxSeeds || HW < 1 || HW > 1 << 22) return fail(SDXL_ERR_INVALID, "cfg_rescale_factors: n (1..8) or HW (1..2^22) out of range");
  if (!(rescale >= 0.f && rescale <= 1.f)) return fail(SDXL_ERR_INVALID, "guidance: rescale must be a finite value in [0, 1]");
  API_BEGIN
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  CfgScales k{};
  for (int b = 0; b < n; ++b) k.v[b] = scales[b];
  Tmp tmp;
  float* partials = (float*)tmp.get(cfg_moments_floats(n, HW) * sizeof(float));
  launch_cfg_rescale_factors(eps, DT_F32, 4, n, HW, k, rescale, partials, factors_out, s);
  SDXL_HIP(hipStreamSynchronize(s));     // the scratch goes away with this call
  API_END
}
// the trajectory without the UNet: a StepLoop of its own, driven as Diffuser::diffuse drives its one, with eps where the UNet's output would be
int sdxl_sampler_step_replay(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* a) {
  return sdxl_sampler_step_replay_pred(ctx, stream, a, SDXL_PREDICTION_EPSILON);
}
int sdxl_sampler_step_replay_pred(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* a, int prediction) {
  return sdxl_sampler_step_replay_ts(ctx, stream, a, prediction, nullptr, 0);
}
// what every replay entry checks besides its schedule
static const char* replay_args_error(const sdxl_ctx* ctx, const sdxl_step_replay_args* a) {
  if (!ctx || !a || !a->eps || !a->latent0 || !a->latents_out || !a->unet_in_out || !a->timesteps_out) return "null argument";
  if (a->n < 1 || a->n > kMaxSeeds || a->h < 1 || a->w < 1 || (int64_t)a->h * a->w > 1 << 22) return "step_replay: n (1..8) or h * w (1..2^22) out of range";
  return nullptr;
}
// the replay itself on a schedule its entry has checked; hist2_out: kSolverDpmpp3M's second history (may be null)
static int replay_run(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* a, int prediction, const std::vector<double>& alphas, const Schedule& sc,
                      float* hist2_out) {
  if ((a->mask != nullptr) != (a->reference != nullptr)) return fail(SDXL_ERR_INVALID, "inpainting needs reference and mask");
  if (a->mask && !a->seeds && !a->step_noise) return fail(SDXL_ERR_INVALID, "inpainting with explicit noise needs step_noise");
  if (!a->seeds && a->eta != 0.0) return fail(SDXL_ERR_INVALID, "eta needs seeds: explicit noise carries none for the sigma term");
  const Guidance g = to_guidance(a->guidance);
  if (const char* m = Diffuser::guidance_error(g, a->single != 0)) return fail(SDXL_ERR_INVALID, m);
  if (g.n_scales != 0 && g.n_scales != a->n) return fail(SDXL_ERR_INVALID, "guidance: n_scales differs from the batch (n)");
  API_BEGIN
  const int n_train = (int)alphas.size();
  if (!a->seeds)      // a table that re-noises (c_z != 0) has no noise to take: refused here, before the device is touched
    if (const char* m = Diffuser::explicit_noise_error(alphas.data(), n_train, sc, a->solver, prediction)) throw InvalidArgumentError(m);
  use(ctx);
  hipStream_t s = pick(ctx, stream);
  const bool single = a->single != 0 || g.mode == kGuidanceOff;
  const int n = a->n, HW = a->h * a->w, B = single ? n : 2 * n;
  const size_t elems = (size_t)n * 4 * HW, bytes = elems * sizeof(float);
  const int in_dt = a->input_f16 ? DT_F16 : DT_F32;
  Tmp tmp;
  StepIo io{};
  io.latent = (float*)tmp.get(bytes);
  io.unet_in = tmp.get((size_t)B * HW * 4 * sizeof(float)); io.in_dt = in_dt;
  io.reference = a->reference; io.mask = a->mask; io.step_noise = a->step_noise; io.seeds = a->seeds;
  SDXL_HIP(hipMemcpyAsync(io.latent, a->latent0, bytes, hipMemcpyDeviceToDevice, s));
  StepLoop loop;
  const int iters = loop.begin(alphas, sc, a->solver, a->eta, a->unconditional_guidance_scale, g, single, n, HW, io, s, prediction);
  for (int i = 0; i <= iters; ++i) {
    if (i > 0) loop.after_forward(i - 1, a->eps + (size_t)(i - 1) * B * HW * 4, s);
    SDXL_HIP(hipMemcpyAsync(a->latents_out + (size_t)i * elems, io.latent, bytes, hipMemcpyDeviceToDevice, s));
    SDXL_HIP(hipMemcpyAsync(a->timesteps_out + i, loop.t_dev(), sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  const bool hist = a->solver == SDXL_SOLVER_DPMPP_2M || a->solver == SDXL_SOLVER_DPMPP_3M;
  if (hist && a->hist_out && iters > 0) SDXL_HIP(hipMemcpyAsync(a->hist_out, loop.hist(), bytes, hipMemcpyDeviceToDevice, s));
  // the second history holds a value only once an update has shifted one into it: with fewer than two iterations it was never written
  if (a->solver == SDXL_SOLVER_DPMPP_3M && hist2_out && iters > 1) SDXL_HIP(hipMemcpyAsync(hist2_out, loop.hist2(), bytes, hipMemcpyDeviceToDevice, s));
  launch_copy_rows(io.unet_in, in_dt, 4, a->unet_in_out, DT_F32, 4, B * HW, 4, s);
  SDXL_HIP(hipStreamSynchronize(s));     // the loop and the scratch go away with this call
  API_END
}
int sdxl_sampler_step_replay_ts(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* a, int prediction, const int32_t* timesteps, int n_ts) {
  if (const char* m = replay_args_error(ctx, a)) return fail(SDXL_ERR_INVALID, m);
  if (a->solver == SDXL_SOLVER_DPMPP_3M && a->alphas_cumprod_host) return fail(SDXL_ERR_INVALID, kSolver3MEntry);
  const bool listed = timesteps != nullptr && n_ts != 0;      // else the reference's rule on the struct's n_steps and step_start
  std::vector<int> ts;
  if (listed) {
    if (const char* m = list_args_error(a->alphas_cumprod_host, a->n_train_steps, timesteps, n_ts, a->solver, a->eta)) return fail(SDXL_ERR_INVALID, m);
    ts.assign(timesteps, timesteps + n_ts);
  } else {
    if (const char* m = schedule_args_error(a->alphas_cumprod_host, a->n_train_steps, a->n_steps, a->step_start, a->solver, a->eta)) return fail(SDXL_ERR_INVALID, m);
    if (a->solver == SDXL_SOLVER_LCM && a->eta != 0.0) return fail(SDXL_ERR_INVALID, "solver LCM takes no eta: eta must be 0 (SDXL_SOLVER_LCM)");
    ts = Diffuser::step_schedule(a->n_steps, a->step_start, a->n_train_steps);
  }
  if (const char* m = alphas_error_pred(a->alphas_cumprod_host, a->n_train_steps, ts, prediction)) return fail(SDXL_ERR_INVALID, m);
  const std::vector<double> alphas(a->alphas_cumprod_host, a->alphas_cumprod_host + a->n_train_steps);   // elem -> f64 as the Diffuser holds them
  Schedule sc;
  try { sc = Diffuser::schedule_of_timesteps(alphas.data(), a->n_train_steps, ts.data(), (int)ts.size()); }
  catch (const std::exception& e) { return fail(SDXL_ERR_INVALID, e.what()); }
  return replay_run(ctx, stream, a, prediction, alphas, sc, nullptr);
}
int sdxl_sampler_step_replay_levels(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* a, int prediction, const sdxl_schedule_desc* schedule,
                                    float* hist2_out) {
  if (const char* m = replay_args_error(ctx, a)) return fail(SDXL_ERR_INVALID, m);
  std::vector<double> alphas;
  Schedule sc;
  if (const char* m = desc_schedule(schedule, a->solver, a->eta, prediction, alphas, sc)) return fail(SDXL_ERR_INVALID, m);
  return replay_run(ctx, stream, a, prediction, alphas, sc, hist2_out);
}
int sdxl_diffuser_enable_step_timing(sdxl_diffuser* d, int enabled) {
  API_BEGIN
  SDXL_REQUIRE(d != nullptr, "null argument");
  d->d->time_steps = enabled != 0;
  API_END
}
int sdxl_diffuser_set_trace(sdxl_diffuser* d, float* trace_dev, int capacity_steps) {
  API_BEGIN
  SDXL_REQUIRE(d && (trace_dev || capacity_steps == 0) && capacity_steps >= 0, "bad argument");
  d->d->trace = capacity_steps > 0 ? trace_dev : nullptr;
  d->d->trace_cap = capacity_steps;
  API_END
}
int sdxl_diffuser_step_times(sdxl_diffuser* d, float* out_ms, int capacity) {
  if (!d || !out_ms) return -1;
  const int n = (int)d->d->step_ms.size() < capacity ? (int)d->d->step_ms.size() : capacity;
  for (int i = 0; i < n; ++i) out_ms[i] = d->d->step_ms[i];
  return n;
}

// ---------------------------------------------------------------------------------------------- VAE
int sdxl_vae_create_f16(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, const uint16_t* dec_w, const uint16_t* enc_w, sdxl_vae** out) {
  API_BEGIN
  vae_create_flat<FlatSourceF16>(ctx, cfg, dtype, dec_w, enc_w, out);
  API_END
}
int sdxl_vae_create(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, const float* dec_w, const float* enc_w, sdxl_vae** out) {
  API_BEGIN
  vae_create_flat<FlatSource>(ctx, cfg, dtype, dec_w, enc_w, out);
  API_END
}
int sdxl_vae_create_synthetic(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, uint64_t seed, int with_encoder, sdxl_vae** out) {
  API_BEGIN
  SDXL_REQUIRE(ctx && out, "bad argument");
  use(ctx);
  int cdt; vae_dtype(dtype, cdt);
  SyntheticSource src(seed);
  vae_create_impl(ctx, to_vcfg(cfg), cdt, &src, with_encoder ? &src : nullptr, out);
  API_END
}
void sdxl_vae_destroy(sdxl_vae* v) {
  if (!v) return;
  delete v->v;
  delete v;
}
int sdxl_vae_decode_latent(sdxl_vae* v, void* stream, const float* latent, int n, int h, int w, float* out) {
  API_BEGIN
  SDXL_REQUIRE(v && latent && out, "null argument");
  use(v->ctx);
  v->v->decode_nchw(latent, n, h, w, out, pick(v->ctx, stream));
  API_END
}
int sdxl_latent_to_image(sdxl_vae* v, void* stream, const float* latent, int n, int h, int w, uint8_t* out) {
  API_BEGIN
  SDXL_REQUIRE(v && latent && out, "null argument");
  use(v->ctx);
  v->v->latent_to_image(latent, n, h, w, out, pick(v->ctx, stream));
  API_END
}
int sdxl_vae_encode_image(sdxl_vae* v, void* stream, const float* image, int n, int H, int W, float* out) {
  API_BEGIN
  SDXL_REQUIRE(v && image && out, "null argument");
  SDXL_REQUIRE(H % 8 == 0 && W % 8 == 0, "image size must be a multiple of 8");
  use(v->ctx);
  v->v->encode_nchw(image, n, H, W, out, pick(v->ctx, stream));
  API_END
}
int sdxl_image_to_latent(sdxl_vae* v, void* stream, const uint8_t* image, int n, int H, int W, float* out) {
  API_BEGIN
  SDXL_REQUIRE(v && image && out, "null argument");
  SDXL_REQUIRE(H % 8 == 0 && W % 8 == 0, "image size must be a multiple of 8");
  use(v->ctx);
  v->v->image_to_latent(image, n, H, W, out, pick(v->ctx, stream));
  API_END
}
int sdxl_vae_weight_arena(sdxl_vae* v, void** base, size_t* bytes) {
  API_BEGIN
  SDXL_REQUIRE(v && base && bytes, "null argument");
  *base = v->v->weight_base(); *bytes = v->v->weight_bytes();
  API_END
}

// ---------------------------------------------------------------------------------------------- weight broadcast (comm.cpp)
void sdxl_set_last_error_(const char* msg) { g_err = msg ? msg : ""; }
int sdxl_unet_bcast_weights(sdxl_comm* comm, sdxl_unet* u, int root) {
  if (!comm || !u) return fail(SDXL_ERR_RUNTIME, "null argument");
  return sdxl_bcast_buffer(comm, nullptr, u->u->weight_base(), u->u->weight_bytes(), root);
}
int sdxl_vae_bcast_weights(sdxl_comm* comm, sdxl_vae* v, int root) {
  if (!comm || !v) return fail(SDXL_ERR_RUNTIME, "null argument");
  return sdxl_bcast_buffer(comm, nullptr, v->v->weight_base(), v->v->weight_bytes(), root);
}
int sdxl_clip_bcast_weights(sdxl_comm* comm, sdxl_clip* c, int root) {
  if (!comm || !c) return fail(SDXL_ERR_RUNTIME, "null argument");
  return sdxl_bcast_buffer(comm, nullptr, c->c->weight_base(), c->c->weight_bytes(), root);
}

}  // extern "C"
