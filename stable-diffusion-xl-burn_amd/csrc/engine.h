// Host-side engine of the MI355X SDXL sampler: parameter enumeration, weight packing into a device arena,
// static per-shape execution plans (bump-allocated activation arena -> stable addresses -> hipGraph replay),
// UNet / VAE / DDIM sampler drivers.  The C ABI in capi.cpp is a thin shell over these classes.
#pragma once
#include "kernels.h"

#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace sdxl {

struct Error : std::runtime_error {
  explicit Error(const std::string& m) : std::runtime_error(m) {}
};
struct InvalidArgumentError : Error {     // an argument the call refuses before anything is launched: SDXL_ERR_INVALID at the C ABI
  explicit InvalidArgumentError(const std::string& m) : Error(m) {}
};
#define SDXL_HIP(x)                                                                                   \
  do {                                                                                                \
    hipError_t e__ = (x);                                                                             \
    if (e__ != hipSuccess) throw ::sdxl::Error(std::string(#x) + " failed: " + hipGetErrorString(e__)); \
  } while (0)
#define SDXL_REQUIRE(cond, msg)                          \
  do {                                                   \
    if (!(cond)) throw ::sdxl::Error(std::string(msg));  \
  } while (0)

static inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------ configs / specs
// mirrors the reference's UNetConfig (unet/mod.rs:59-69) + DiffuserConfig.is_refiner (stablediffusion/mod.rs:269-278)
struct UNetCfg {
  int adm_in_channels = 0, in_channels = 4, out_channels = 4, model_channels = 0;
  std::vector<int> channel_mults;
  int n_head_channels = 64;
  std::vector<int> transformer_depths;
  int context_dim = 0;
  bool is_refiner = false;
};
// AutoencoderConfig::init hard-codes the SDXL values (autoencoder/mod.rs:27-35); kept configurable for tiny tests
struct VaeCfg {
  std::vector<std::pair<int, int>> enc{{128, 128}, {128, 256}, {256, 512}, {512, 512}};
  std::vector<std::pair<int, int>> dec{{512, 512}, {512, 512}, {512, 256}, {256, 128}};
  int n_group = 32;
  int enc_out = 8;
  double scale_factor = 0.13025;
};

// mirrors CLIPConfig (clip/mod.rs:19-28)
struct ClipCfg { int n_vocab = 49408, n_state = 0, embed_dim = 0, n_head = 0, n_ctx = 77, n_layer = 0; bool quick_gelu = false; };

enum ParamKind { PK_LINEAR_W = 0, PK_CONV_W = 1, PK_BIAS = 2, PK_GAMMA = 3, PK_BETA = 4, PK_EPS = 5 };
struct ParamSpec {
  std::string name;
  std::vector<int> shape;
  int kind;
  float scale, mean;   // synthetic init: value = (u - 0.5)*scale + mean
  size_t numel() const { size_t n = 1; for (int d : shape) n *= (size_t)d; return n; }
};
enum BlockKind { BK_CONV, BK_RES, BK_DOWN, BK_REST, BK_RESTU, BK_RESU };
struct BlockDesc { int kind = 0, c_in = 0, c_emb = 0, c_out = 0, n_head = 0, depth = 0; };
void unet_block_plan(const UNetCfg& cfg, std::vector<BlockDesc>& inp, BlockDesc& mid, std::vector<BlockDesc>& out);
std::vector<ParamSpec> unet_param_specs(const UNetCfg& cfg);
// a ControlNet for the UNet `unet` (sdxl_controlnet_config): that UNet's encoder + hint embedder + one 1x1 convolution per residual tensor
struct ControlCfg { UNetCfg unet; int hint_in = 3; int hint_channels[4] = {16, 32, 96, 256}; };
std::vector<ParamSpec> controlnet_param_specs(const ControlCfg& cfg);
std::vector<ParamSpec> vae_decoder_param_specs(const VaeCfg& cfg);
std::vector<ParamSpec> vae_encoder_param_specs(const VaeCfg& cfg);
std::vector<ParamSpec> clip_param_specs(const ClipCfg& cfg);
uint64_t fnv1a64(const std::string& s);

// ------------------------------------------------------------------------------------------ memory
struct DeviceArena {
  char* base = nullptr;
  size_t cap = 0, off = 0, peak = 0;
  bool dry = false;     // dry run: hand out offsets from a null base, only track the peak
  ~DeviceArena();
  void reserve(size_t bytes);
  void* alloc(size_t bytes);
  size_t mark() const { return off; }
  void reset(size_t m) { off = m; }
};

// where canonical (reference-layout fp32) parameter tensors come from
struct WeightSource {
  virtual ~WeightSource() {}
  virtual void fetch(const ParamSpec& s, size_t index, float* dst_dev, hipStream_t st) = 0;
  virtual bool empty() const { return false; }   // true: lay the arena out but leave its contents to a later broadcast
};
struct NullSource : WeightSource {   // replica ranks: same arena layout, contents arrive by RCCL broadcast from rank 0
  void fetch(const ParamSpec&, size_t, float*, hipStream_t) override {}
  bool empty() const override { return true; }
};
constexpr float kHiLoScale = 256.0f;    // lo halves of the LF_F16_WHILO packing travel times 2^8 (out of the f16 subnormals), the A operand's second copy times 2^-8
constexpr uint64_t kSeedF16Weights = 1ull << 63;   // seed flag (C ABI: SDXL_SEED_F16_WEIGHTS): synthetic parameters rounded to f16
struct SyntheticSource : WeightSource {
  uint64_t seed;
  explicit SyntheticSource(uint64_t s) : seed(s) {}
  void fetch(const ParamSpec& s, size_t index, float* dst_dev, hipStream_t st) override;
};
struct FlatSource : WeightSource {   // flat fp32 buffer (host or device) in spec order
  const float* base; std::vector<size_t> offsets;
  FlatSource(const float* b, const std::vector<ParamSpec>& specs);
  void fetch(const ParamSpec& s, size_t index, float* dst_dev, hipStream_t st) override;
};

struct FlatSourceF16 : WeightSource {   // flat IEEE-f16 buffer (host or device) in spec order -- how burn's HalfPrecisionSettings
  // records store the weights (src/bin/sample/main.rs:37, src/bin/convert/main.rs:65-70): half the host memory of the fp32 path
  const uint16_t* base; std::vector<size_t> offsets;
  void* stage = nullptr; size_t stage_numel = 0;
  FlatSourceF16(const uint16_t* b, const std::vector<ParamSpec>& specs);
  ~FlatSourceF16() override;
  void fetch(const ParamSpec& s, size_t index, float* dst_dev, hipStream_t st) override;
};

// Create-time adapters (C ABI: sdxl_lora_entry): W += scale * left @ right on the matrix view of a PK_LINEAR_W / PK_CONV_W parameter,
// rows = shape[0], cols = product of the other dimensions; left [rows, rank], right [rank, cols], fp32, host or device.  In terms of the usual
// PyTorch adapter tensors (down.weight [r, in...], up.weight [out, r]):
//   PK_LINEAR_W [d_in, d_out]:      left = down.weight^T,  right = up.weight^T
//   PK_CONV_W   [Cout, Cin, kh, kw]: left = up.weight,      right = down.weight flattened to [r, Cin * kh * kw]
struct LoraEntry { int param_index = 0, rank = 0; const float* left = nullptr; const float* right = nullptr; float scale = 0.f; };
constexpr int kLoraRoundF16 = 1;      // C ABI: SDXL_LORA_ROUND_F16
// empty string: every entry names a PK_LINEAR_W / PK_CONV_W parameter of specs, rank >= 1, non-null arrays, finite scale; else the first complaint (host logic only)
std::string lora_check(const std::vector<ParamSpec>& specs, const LoraEntry* entries, int n_entries);
// A source that wraps another one: fetch() asks the inner source, then merges every entry of that parameter into dst_dev in the order the entries were
// given (launch_lora_merge: several adapters on one tensor stack), last -- kLoraRoundF16 -- rounds the adapted tensor to f16 values (what a half-precision
// record saved after merging holds).  It sits in front of WeightBuilder, so every packing form, every dtype and the f16-exactness guard
// (WeightBuilder::all_f16_exact) see the merged tensor; nothing downstream knows adapters exist.  The entries' arrays are staged per fetch into a
// device buffer this source owns; they must stay alive while the model is built.
struct LoraSource : WeightSource {
  WeightSource& inner;
  std::vector<LoraEntry> entries;
  std::vector<std::vector<int>> by_param;      // entry indices per parameter, in the order given
  int flags;
  float* stage = nullptr; size_t stage_numel = 0;
  LoraSource(WeightSource& in, const std::vector<ParamSpec>& specs, const LoraEntry* e, int n_entries, int flags);
  ~LoraSource() override;
  void fetch(const ParamSpec& s, size_t index, float* dst_dev, hipStream_t st) override;
  bool empty() const override { return inner.empty(); }
};

struct Lin {        // packed dense weight: [Npad][Kpad] compute dtype + fp32 bias [Npad]
  const void* w = nullptr; const float* b = nullptr;
  const void* wf = nullptr;        // f16 linear layers / 1x1 convs with N % 128 == 0: the same weights in MFMA fragment order (igemm_wreg.hip)
  int N = 0, K = 0, Kpad = 0, Npad = 0, ksize = 1, cin = 0;
  // a LayerNorm in front (LnMode): cs = column sums of the packed rows (LN_FOLD) or gamma W over them (LN_SHADOW), b = beta W + bias; the GEMM
  // then takes the RAW rows plus their per-64-column (mean, M2) statistics -- see IgemmParams::ln_stat
  const float* cs = nullptr;
  const float* ln_eps = nullptr;   // device scalar: eps of the folded LayerNorm
  int ln_k = 0;                    // folded LayerNorm over ln_k columns (0: K) -- the (hi | lo) shadow form packs K = 2 ln_k
  int k_form = 0;                  // 0 plain; 1: K doubled as two HALVES, weight (hi | lo s) or (w | w / s) against [a | a / s] or [a_hi | a_lo s] (LF_F16_WHILO / _AHILO); 2: K doubled in the HL16
                                   // interleave, the weight twice per 16-channel group: the A operand is an un-scaled HL16 tensor read as f16 (MIX_LINEAR_F16X2)
  int dt = -1;                     // dtype the weight was packed in when it differs from the model's compute dtype (-1: the model's):
                                   // a DT_HL model packs the layers its pipeline cannot take (Cin % 32 != 0) as fp32
  const float* acc_scale = nullptr;   // DT_HL packing: device scalar (weight arena) 1 / (power-of-two factor the packed weights carry)
  // 3x3 convolutions behind a nearest-2x upsample (WeightBuilder::conv fold_up): the four 2x2-tap phase matrices of upsample + conv (upsample_fold.h),
  // [4][Npad][4 cin] packed like w, with their own accumulator scale (the sums of up to four taps have their own range).  run_conv takes them where the
  // caller allows it (Epi::fold) and the launch fits the phase form (IgemmParams::ph_rows); null: the layer has the gather form only
  const void* w_fold = nullptr; const float* fold_acc_scale = nullptr;
};
// eps lives in the weight arena (device scalar, read by the kernels): replicas that receive the arena by broadcast need no
// host-side copy, and a checkpoint's per-norm eps (groupnorm/load.rs:19, layernorm/load.rs:17) travels with the weights
struct NormW { const float* gamma = nullptr; const float* beta = nullptr; const float* eps = nullptr; int C = 0; };

// Form of a transformer projection on a split-operand model (StPlan): what it packs and which operand it reads
enum LinForm {
  LF_NATIVE,      // split-operand (HL16) weights, fp32-class (fp32 where K % 32 != 0)
  LF_F16,         // plain f16 weights x f16 operand
  LF_F16_WHILO,   // (hi | lo 2^8) weight halves along a doubled K against [a | a 2^-8] (MIX_GEGLU_HILO; k_form 1)
  LF_F16_AHILO,   // (w | w 2^-8) against (hi | lo 2^8) activation halves (MIX_GEGLU_AHILO; k_form 1)
  LF_X2           // the weight twice in the HL16 interleave against an HL16 operand read as f16 (MIX_LINEAR_F16X2; k_form 2)
};
inline bool packs_f16_values(LinForm f) { return f == LF_F16 || f == LF_F16_AHILO || f == LF_X2; }   // the packed weights are the parameter rounded to f16
// How a preceding LayerNorm(gamma, beta) enters a projection:  LN(x) W + b = rstd (x - mu) (diag(gamma) W) + (beta W + b)
//   = rstd * (x W') - rstd * mu * colsum(W') + b'   -- the GEMM takes the RAW rows plus their row statistics (IgemmParams::ln_stat)
enum LnMode {
  LN_NONE,        // not at all: the projection reads the output of a LayerNorm launch (or no LayerNorm)
  LN_FOLD,        // folded into the weight (the f16 engine): W' = diag(gamma) W packed (rounded to the compute dtype) FIRST, cs = column sums over the
                  // rounded values -- the identity holds exactly for what the MFMA multiplies --, b = beta W + bias
  LN_SHADOW       // shadow form (split-operand models, MIX_LN_SHADOW): the weight stays UN-folded in f16 (an f16-valued parameter stays exact), gamma rides on
                  // the A operand -- the shadow f16(x o gamma) the producer of the fp32 stream leaves (IgemmParams::shadow) --, cs = gamma W over the packed
                  // values, b = beta W + bias; a plain twin shares the packed matrix and has the canonical bias (the LayerNorm-launch path)
};
// One [K,N] projection, or several fused along N, as WeightBuilder::pack takes it
struct Proj {
  std::vector<std::string> names;       // name.weight [K,N] (+ name.bias); several: concatenated along N (same K), ONE DT_HL scale for the matrix
  bool geglu = false;                   // columns interleaved (16 x | 16 gate) for the GEGLU epilogue; a single projection
  int dt = -1;                          // packed dtype whatever the model's (the GEMV weights of a split-operand model stay fp32); -1: the model's
  LinForm form = LF_NATIVE;             // LF_NATIVE: plain, in the model's dtype or `dt`; LF_F16: plain f16; the doubled-K forms are f16 and need K % 32 == 0
  LnMode ln = LN_NONE; std::string norm;      // the LayerNorm in front (its parameter prefix)
  bool wfrag_folded = false;            // LN_FOLD: also the fragment-order image (the attn2 query projection: the weights-in-registers kernel applies the
                                        // folded affine in its fused cross-attention form alone)
  Lin* shadow = nullptr;                // LN_SHADOW: receives the shadow form (.cs set); pack() returns its plain twin
};

// dt_override of the M <= 8 GEMV weights (time / label MLPs, the hoisted lin_embed) for a model of compute dtype cdt: a split-operand model packs them
// fp32 (gemv_kernel reads f16 or fp32 rows, not HL16), every other model in its own dtype (-1).  One rule for UNet's constructor and sdxl_gemv.
inline int gemv_weight_dt(int cdt) { return cdt == DT_HL ? DT_F32 : -1; }

struct WeightBuilder {
  const std::vector<ParamSpec>& specs;
  std::map<std::string, size_t> index;
  WeightSource& src;
  DeviceArena& arena;
  int dt;
  hipStream_t st;
  float* tmp = nullptr; size_t tmp_numel = 0;      // staging buffer of fetch(), allocated on the first one (a layout pass makes no device call)
  std::string last_fetched;      // name of the tensor `tmp` holds (fetch() of the same name again is free)
  WeightBuilder(const std::vector<ParamSpec>& sp, WeightSource& s, DeviceArena& a, int dtype, hipStream_t stream);
  ~WeightBuilder();
  // wfrag: the model keeps fragment-order images of its plain f16 linear / 1x1 weights (alloc_wfrag) -- only the UNet's layers can be
  // routed to the weights-in-registers kernel, so the CLIP towers and the VAE leave it off (half the arena / broadcast bytes for those layers)
  bool wfrag = true;
  const ParamSpec& spec(const std::string& name, size_t* idx = nullptr) const;
  bool has(const std::string& name) const { return index.count(name) != 0; }
  const float* fetch(const std::string& name);            // canonical fp32 tensor in tmp
  // Every routine below has two phases in one body.  LAYOUT runs always: every arena.alloc of the layer, in one fixed order.  FILL is skipped as a
  // whole when src.empty().  So an empty source lays out the identical arena -- replica ranks receive rank 0's by broadcast -- and over a dry
  // arena it is the pass that sizes the reservation (UNet / Vae / ClipText run their loader twice).
  // pack: the one routine for projections.  Allocation order (run_conv's weight warming extends a launch's cold region over these neighbours):
  //   packed weights [Npad][Kpad], bias [Npad], [DT_HL: scale + exactness flag], [LN_FOLD / LN_SHADOW: column sums [Npad], eps],
  //   [LN_SHADOW: the plain twin's bias [Npad]], [fragment-order image]
  // Fragment image: never for a fused matrix, a GEGLU projection or a shadow pair; a doubled-K form only LF_X2; a folded weight only with
  // wfrag_folded; and then only where alloc_wfrag's shape rule holds.  DT_HL falls back to fp32 where K % 32 != 0; k-tiles of 64 (f16) / 32.
  Lin pack(const Proj& p);
  Lin linear(const std::string& name, bool geglu = false, int dt_override = -1) { Proj p; p.names = {name}; p.geglu = geglu; p.dt = dt_override; return pack(p); }
  Lin fused_linear(const std::vector<std::string>& names, int dt_override = -1) { Proj p; p.names = names; p.dt = dt_override; return pack(p); }
  // AND of "every value of these tensors is exactly one f16" (device flag read back): what SDXL_DTYPE_F32_SPLIT_MIX_F16W asks of the classes it moves to f16
  bool all_f16_exact(const std::vector<std::string>& names);
  float* tmp2 = nullptr; size_t tmp2_numel = 0;   // scratch for folded biases / folded upsample weights (device)
  // name.weight [Cout,Cin,k,k] + bias.  fold_up: a 3x3 conv that runs behind a nearest-2x upsample also gets its folded phase matrices (Lin::w_fold) where
  // folds_upsample holds; folded from the fetched tensor, i.e. after any adapter merge.
  // Allocation order: packed weights, bias, [DT_HL: scale], [phase matrices], [DT_HL: their scale], [fragment-order image (1x1)]
  Lin conv(const std::string& name, bool fold_up = false);
  static bool folds_upsample(const ParamSpec& p, int dt);     // f16 and split-operand packings of a 3x3 kernel with whole k-tiles per tap
  NormW norm(const std::string& name);                       // gamma [C], beta [C], eps
 private:
  float* need_tmp2(size_t numel);
  // DT_HL packing: two arena floats -- [0] 1 / (power-of-two factor of the packed weights), [1] "every weight is one f16" --, filled by hl_scale (-> the factor)
  // over every tensor `each` visits
  template <typename Each> float hl_scale(float* sc, Each each);
  bool alloc_wfrag(Lin& l, bool folded = false);    // layout of the second image of a plain f16 linear / 1x1 weight in fragment order (no-op for other layers)
};

// activation view: rows of `ld` elements
struct Act {
  void* p = nullptr; int ld = 0; int dt = DT_F16;
  // GroupNorm statistics of this tensor left behind by the GEMM that produced it (Epi::gn_part -> IgemmParams::gn_part):
  // [B][gn_rt][C] (mean, M2) per 256-row tile and channel.  A GroupNorm over exactly this tensor skips its statistics pass.
  const float* gn_part = nullptr; int gn_rt = 0;
  const float* a_scale = nullptr;   // HL16 copy of an fp32 stream tensor (hl_operand): 2^-e per batch entry, multiplied back by the consuming GEMM (IgemmParams::a_scale)
  int a_scale_n = 1;                // entries of a_scale (equal row counts each)
  Act() {}
  Act(void* p_, int ld_, int dt_) : p(p_), ld(ld_), dt(dt_) {}
  Act cols(int c0) const { Act a((char*)p + (size_t)c0 * dt_size(dt), ld, dt); a.a_scale = a_scale; a.a_scale_n = a_scale_n; return a; }   // (a column slice drops the statistics)
};

// per-kernel-class hipEvent profiler (eager runs only): live measurement of the dominant kernel for bench.py's roofline
struct Profiler {
  enum { IGEMM = 0, ATTENTION = 1, GROUPNORM = 2, LAYERNORM = 3, OTHER = 4, NCLS = 5 };
  struct Rec { hipEvent_t a, b; int cls; double flops; int m, n, k, ks, tag; };
  std::vector<Rec> recs;
  void begin(int cls, double flops, hipStream_t s, int m = 0, int n = 0, int k = 0, int ks = 0, int tag = 0);   // tag: DemoteClass bit of the launch (UNet; 0 = untagged)
  void end(hipStream_t s);
  void collect(float ms[NCLS], int launches[NCLS], double flops[NCLS]);   // synchronises, then frees the events
};

// the GEMM launches of one forward in launch order (weights each one reads, whether its kernel can host warming workgroups):
// recorded on the plan's first eager forward, replayed on every later one -- launch i is handed the weights of a later launch
// (IgemmParams::warm).  Static shapes: the sequence of a plan never changes.
struct WarmSeq {
  struct Item { const void* w; unsigned bytes; bool host; unsigned budget; const void* warm[3]; unsigned warm_bytes[3]; };
  std::vector<Item> seq;
  size_t pos = 0;
  bool recording = false, ready = false;
  void finish();       // assigns targets to hosts (weights.cpp)
};
struct Exec {
  Profiler* prof = nullptr;
  hipStream_t s = nullptr;
  bool dry = false;
  int cdt = DT_F16;      // compute dtype (MFMA operands)
  int sdt = DT_F16;      // residual-stream dtype
  DeviceArena* act = nullptr;
  float* gn_partial = nullptr;
  float* splitk_ws = nullptr; size_t splitk_ws_bytes = 0; unsigned* splitk_cnt = nullptr;   // igemm split-K workspace (optional)
  const float* ebias = nullptr;   // [nb][emb_total] per-ResBlock time-embedding biases of this run's batch entries
  int b0 = 0;                      // first batch entry of this run (split-CFG chains address the K/V caches with it)
  hipEvent_t fork_ev = nullptr;    // split-CFG: recorded on s after the fork_after-th GEMM launch of chain 0 -- the second
  int fork_after = 0, launches = 0; // chain starts there, so the two chains run out of phase (GEMMs of one under the attention of the other)
  WarmSeq* warm = nullptr;         // weight warming schedule of the plan (null: off)
  float* attn_xws = nullptr; unsigned* attn_xcnt = nullptr;   // workspace / tickets of the cross-workgroup key split (AttnParams::xws)
  int demote = 0;                  // split-operand UNet, precision-frontier instrument: GEMM classes (DemoteClass bits) whose operands lose their lo halves
  Act alloc(size_t rows, int C, int dt) {
    return Act(act->alloc(rows * (size_t)C * dt_size(dt)), C, dt);
  }
};

// Precision-frontier instrument (round 5; sdxl_debug_set "hl_demote" = bit set).  A split-operand (DT_HL) UNet runs the GEMMs of the listed
// classes on operands whose lo halves are zero -- activations by a zeroing pass behind their producer, weights through the "every weight is
// one f16" flag of the packed matrix (IgemmParams::acc_scale[1]: the kernel leaves the w_lo MFMAs out), the attention through
// AttnParams::demote -- i.e. with exactly the f16 engine's operand rounding (f16 x f16 products, fp32 accumulation) while every other class
// keeps fp32-class operands.  Measures each class's share of the f16 mode's error on the config-2 trajectory (tools/precision_frontier.py).
// Classes: self-attention QKV projection, the self-attention itself (q, k, v, p), attention out-projections, cross-attention (query / key / value
// projections + the 77-key attention), GEGLU projection, FF-out, and five kinds of convolution: the two 3x3 convs of every ResBlock, the 1x1 skip
// connections, the UNet's last conv (its first has 4 input channels and is plain fp32 in this engine), the down / up-sampling convs, proj_in / proj_out.
// SDXL_DTYPE_F32_SPLIT_MIX: what the measured frontier (profiles/r05_precision_frontier.json) lets a latents-within-bound engine run in f16
// (classes 4 ... 32: SDXL_DTYPE_F32_SPLIT_MIX_F16W, or sdxl_debug_set "mix_classes" -- outside the bound on the synthetic fp32 weights, inside it on
//  f16-representable ones)
enum MixClass {
  MIX_ATTN_F16 = 1,     // self-attention on the f16 flash kernels
  MIX_GEGLU_F16 = 2,    // GEGLU projection (f16 LayerNorm output x f16 weights)
  MIX_QKV_F16 = 4,      // QKV projection (implies the f16 self-attention)
  MIX_FF_F16 = 8,       // FF-out (reads the GEGLU kernel's f16 output)
  MIX_OUT1_F16 = 16,    // self-attention out-projection (reads the f16 attention output as it is)
  MIX_OUT2_F16 = 32,    // cross-attention out-projection (the split-operand attention rounds its fp32 result to f16 once, in its store)
  MIX_XATTN_F16 = 64,   // with OUT2: cross-attention + its query projection as the f16 engine's fused launch -- a knob, in no mode
  MIX_Q2_F16 = 128,     // cross-attention QUERY projection alone on f16 operands (HL16 output: the split-operand attention behind it keeps an fp32-class q)
  MIX_XATTN_SPLIT = 512, // with MIX_Q2_F16 + MIX_OUT2_F16, or MIX_LINEAR_F16X2: the 77-key cross-attention at SPLIT precision inside the f16 query projection's epilogue (IgemmParams::xa_k_lo) -- the
                        // arithmetic of the stand-alone split-operand attention without its launch
  MIX_GEGLU_HILO = 1024, // with MIX_GEGLU_F16 (and without the shadow form): the GEGLU weights as (hi, lo) f16 pairs along a doubled K against [a | a 2^-8] -- the f16 wide-tile
                        // kernel at twice the depth, two MFMAs per product: activation rounding only on ANY weights.  SDXL_DTYPE_F32_SPLIT_MIX
  MIX_GEGLU_AHILO = 2048, // with MIX_GEGLU_F16 (f16-representable weights): the GEGLU projection's ACTIVATIONS as (hi, lo) f16 pairs along a doubled K against (w | w 2^-8) --
                        // the class that carries 70 % of the F16W mode's error variance at two MFMAs per product on the f16 kernel.  SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2
  MIX_LINEAR_F16X2 = 4096, // (f16-representable weights) transformer linears whose A operand is an un-scaled HL16 tensor run on the F16 kernels: an HL16 row of C channels is an f16 row of 2 C
                        // columns, the weight is packed twice in the same interleave -- two MFMAs per product on the weights-in-registers / wide / pipe kernels
  MIX_LN_SHADOW = 256   // the LayerNorms in front of the f16 projections (QKV, GEGLU, the query projection; f16 or MIX_LINEAR_F16X2) folded into them: the producers of
                        // the fp32 stream leave an f16 shadow f16(x o gamma) + row statistics (IgemmParams::shadow), no LayerNorm launch
};
enum DemoteClass { DM_QKV = 1, DM_ATTN = 2, DM_OUT = 4, DM_XATTN = 8, DM_GEGLU = 16, DM_FF = 32, DM_CONV_RES = 64, DM_CONV_SKIP = 128,
                   DM_CONV_IO = 256, DM_CONV_UPDOWN = 512, DM_CONV_PROJ = 1024 };
void unet_set_mix_classes(int v);
void unet_set_hl_demote(int mask);
void unet_set_xattn_long(int v);     // A/B knob (sdxl_debug_set "xattn_long", default 1): 0 = contexts above 96 keys keep the un-fused cross-attention; read by UNet::set_context
int unet_hl_demote();

// thin launch helpers shared by unet.cpp / vae.cpp (skip the launch on dry runs)
struct ConvGeom { int B, Hin, Win, Hout, Wout, ksize, stride, pad, up; };
struct Epi {
  const float* ln_stat = nullptr;   // [K/64][M][2] per-slot (mean, M2) of the A rows: the weight is LayerNorm-folded (Lin::cs)
  float* stat_out = nullptr;        // [N/64][M][2]: leave the per-slot (mean, M2) of the output rows for the next folded LayerNorm
  const float* ebias = nullptr; int ebias_ld = 0;
  int act = 0;
  Act R;             // residual (p == nullptr -> none)
  int n_split = -1;  // >=0: columns >= n_split go transposed into Ct
  void* Ct = nullptr; int ct_rows = 0, ct_ld = 0;
  int rpb = 0;       // rows per batch for ebias / transposed store (0 -> Hout*Wout)
  // cross-attention fused into the projection's epilogue (IgemmParams::xa_*): packed context of this run's batch entries
  const void* xa_k = nullptr; int xa_nctx = 0; float xa_scale = 0.f;   // xa_k: operand-order image (launch_xattn_pack)
  const void* xa_k_lo = nullptr;     // split precision (IgemmParams::xa_k_lo): xa_k = hi halves, this = lo halves of the context keys / values
  // room for the GroupNorm statistics of the output ([M/256][N] float pairs); run_conv reports whether the kernel it picked
  // filled it (igemm_gn_part_ok), the caller then tags the output Act
  float* gn_part = nullptr;
  bool* fold_done = nullptr;   // (optional) run_conv reports whether the launch took the folded form
  bool fold = false; // an upsample convolution (ConvGeom::up) may run as the four folded phase convolutions (Lin::w_fold) where the launch fits
  int cls = 0;       // DemoteClass bit of this GEMM (UNet call sites): label of the launch in the per-launch profile dump, nothing else
  // f16 shadow of an fp32 output for the GEMM behind the next LayerNorm (IgemmParams::shadow): asked for by the caller, written only when the kernel the
  // selection picks can (weights-in-registers kernel) -- *shadow_done tells; stat_out then holds the fp32 rows' statistics
  void* shadow = nullptr; int shadow_ld = 0; const float* shadow_gamma = nullptr; bool* shadow_done = nullptr; float shadow_lo_scale = 0.f;
};
bool run_conv(Exec& ex, const Lin& w, const Act& a, int cin, const ConvGeom& g, const Act& out, const Epi& e = Epi());   // true: e.gn_part was filled
void set_upsample_fold(int v);     // A/B knob (sdxl_debug_set "upsample_fold", default 1): 0 = every upsample convolution keeps the gather form (read per launch; a captured plan keeps what it recorded)
bool run_linear(Exec& ex, const Lin& w, const Act& a, int M, const Act& out, const Epi& e = Epi());
// have_max: a hl_scale_floats(nb) buffer whose max|x| partials a GroupNorm statistics pass over x already wrote (run_groupnorm absmax_out): no absmax pass
Act hl_operand(Exec& ex, const Lin& w, const Act& x, size_t rows, int C, int nb = 1, float* have_max = nullptr);    // HL16 copy of an fp32 stream tensor (nb batch entries of rows / nb rows, one power-of-two scale each) for a split-operand GEMM (else x)
// absmax_out: hl_scale_floats(B) floats; the statistics pass (fp32 x without producer statistics -- the caller checks) also leaves max|x| partials per entry there
void run_groupnorm(Exec& ex, const NormW& n, const Act& x, int B, int HW, const Act& y, bool silu, int groups = 32, float* absmax_out = nullptr);
void run_layernorm(Exec& ex, const NormW& n, const Act& x, int rows, const Act& y, float dup_scale = 0.f);   // dup_scale: LayerNormParams::dup_scale

// ------------------------------------------------------------------------------------------ UNet
struct ResBlockW { NormW norm_in, norm_out; Lin conv_in, conv_out, skip; bool has_skip = false; int emb_off = 0, cin = 0, cout = 0; };
struct TBlockW { NormW n1, n2, n3; Lin qkv, out1, q2, kv2, out2, geglu, ff;
                 Lin qkv_sh, q2_sh, geglu_sh; };   // *_sh: shadow forms (MIX_LN_SHADOW; .cs set) sharing the packed matrix of their plain twin
enum XattnForm { XA_LAUNCH, XA_F16, XA_SPLIT };   // cross-attention: its own launch / in the query projection's epilogue on f16 (the f16 engines'
                                                  // fused launch; MIX_XATTN_F16) / there at split precision (MIX_XATTN_SPLIT)
// how one spatial transformer runs (UNet plan_transformer): the only reading of the MixClass bits besides the fallback and mix_classes()
struct StPlan {
  LinForm qkv = LF_NATIVE, out1 = LF_NATIVE, q2 = LF_NATIVE, out2 = LF_NATIVE, geglu = LF_NATIVE, ff = LF_NATIVE;
  bool qkv_sh = false, q2_sh = false, geglu_sh = false;   // LayerNorm-shadow twins (MIX_LN_SHADOW)
  bool attn_f16 = false;                                   // self-attention on the f16 flash kernels
  XattnForm xattn = XA_LAUNCH;                             // (where the forward's shapes and the context images allow it)
};
struct STW { NormW norm; Lin proj_in, proj_out; std::vector<TBlockW> blocks; int C = 0, heads = 0; StPlan plan; };
// The LayerNorm-fed projections of a transformer block, shared by UNet::spatial_transformer and the op entry that runs one of them
// (sdxl_transformer_projection), so that both go through the same packing (WeightBuilder::pack), operands and shadow hand-off.
inline bool reads_f16(LinForm f) { return f == LF_F16 || f == LF_F16_WHILO || f == LF_F16_AHILO; }   // the projection reads f16 activations
// X2: an un-scaled HL16 operand of C logical channels handed to an f16 GEMM whose weight is packed twice in the HL16 interleave (K = 2 C)
inline Act x2_operand(LinForm f, const Act& a) { return f == LF_X2 ? Act(a.p, 2 * a.ld, DT_F16) : a; }
// the operands a LayerNorm launch writes for the forms of plan `pl`, and the shadow the weights-in-registers producers of the stream (out-projections,
// FF-out) leave for the projection behind the next LayerNorm (MIX_LN_SHADOW); `have_sh`: the last producer wrote it (else: LayerNorm launch + the
// plain form of the projection)
struct LnOperands {
  Act ln;                           // LayerNorm output in the compute dtype (NATIVE; X2 reads it as f16 rows of 2 C)
  Act ln16;                         // f16 LayerNorm output (LF_F16)
  Act ln16x2;                       // [a | a 2^-8] (WHILO) or [a_hi | a_lo 2^8] (AHILO) along a doubled K
  Act sh16; float* shst = nullptr;  // f16 shadow f16(x o gamma) + the fp32 rows' statistics
  Act sh16g;                        // (hi | lo 2^8) shadow for a GEGLU projection packed (w | w 2^-8) along a doubled K
  Act shhl;                         // X2 shadow: the HL16 image of x o gamma (the LayerNorm launch's operand minus the normalisation the consumer applies)
  bool have_sh = false;
  size_t M = 0; int C = 0;
};
void alloc_ln_operands(Exec& ex, const StPlan& pl, size_t M, int C, const Act& ln, LnOperands& o);   // ln: the compute-dtype LayerNorm output (allocated by the caller)
void want_ln_shadow(LnOperands& o, Epi& e, bool sh, LinForm f, const NormW& n);     // ask producer `e` for the shadow the consumer (form f) behind LayerNorm n reads
// the projection behind LayerNorm n: its shadow twin on the shadow the producer left (no LayerNorm launch), or its plain form on a LayerNorm launch
// of stream t into the operand the form reads.  -> (weights, operand, row statistics of the shadow)
struct LnIn { const Lin* w; Act a; const float* stat; };
LnIn ln_input(Exec& ex, LnOperands& o, const Lin& plain, const Lin& sh, LinForm f, const NormW& n, const Act& t, int cls);
// the f16 GEGLU kernels store an HL16 output through the LDS-staged epilogue of the wide / pipelined tiles -- the kernels every SDXL shape runs on
// (M = 2048 ... 32768).  Small token counts (tiny test nets: M < 256) run on other tiles; they take the form the F16_F32RES engine runs at every
// size -- f16 output -- and widen it.  true: the GEGLU projection `in` of form f writes f16 rows that are widened afterwards
constexpr size_t kGegluDirectRows = 256;
inline bool geglu_widened(LinForm f, const LnIn& in, size_t M) { return M < kGegluDirectRows && (in.stat || reads_f16(f)); }
struct BlockW { BlockDesc d; ResBlockW res; STW st; Lin conv; };

class UNet {
 public:
  // mix (split-operand compute only): MIX_* classes that run on plain f16 operands instead (SDXL_DTYPE_F32_SPLIT_MIX)
  UNet(const UNetCfg& cfg, int compute_dt, int stream_dt, WeightSource& src, hipStream_t st, int mix = 0);
  ~UNet();
  const UNetCfg& cfg() const { return cfg_; }
  // conditioning that is constant over a trajectory: context [B][n_ctx][ctx_dim] fp32 (device), label [B][adm] fp32.
  // Projects the cross-attention K / V^T of all transformer blocks once (reference recomputes them every step,
  // unet/mod.rs:1010-1011) and the label embedding MLP (:464-466).
  void set_context(const float* context, int n_ctx, const float* label, int B, hipStream_t s);
  // x: NHWC [B][H*W][in_ch] in compute dtype at unet_in(); t: device fp32 per batch entry (stride t_stride);
  // result: NHWC [B][H*W][out_ch] fp32 at eps_out().
  void forward(int B, int H, int W, const float* t_dev, int t_stride, hipStream_t s);
  // reference-shaped entry (unet/mod.rs:450-456): NCHW fp32 in/out, int32 device timesteps
  void forward_nchw(const float* x, const int* timesteps, const float* context, int n_ctx, const float* label,
                    int B, int H, int W, float* out, hipStream_t s);
  // one entry of the block plan on caller tensors (sdxl_unet_block): x NCHW fp32 [B][c_in][h][w] at the entry's own resolution is laid out as the entry's
  // source is in a forward of the top-level size its level implies (row stride of the concat slice / buffer it reads there), the entry runs through
  // run_entry with the ebias slice of the one embcat_ GEMV over emb [B][4 mc] and the caches set_context leaves for context, and its destination (row stride
  // and column offset as in the forward) comes back as NCHW fp32.  out == nullptr: only out_shape {B, C, h, w} is filled, nothing is launched.
  // Replaces the handle's context (label embedding included: the next forward sets its own).  Indices / shapes outside the plan: InvalidArgumentError.
  enum Section { SEC_INPUT = 0, SEC_MIDDLE = 1, SEC_OUTPUT = 2, SEC_HEAD = 3 };
  void run_block(int section, int index, const float* x, const float* emb, const float* context, int n_ctx, int B, int c_in, int h, int w, float* out,
                 int64_t out_shape[4], hipStream_t s);
  // ControlNet skip residuals.  The residual tensors of a UNet: one per input entry (its output shape), then the middle block's.
  struct SkipShape { int C = 0, h = 0, w = 0; };
  static std::vector<SkipShape> skip_shapes(const UNetCfg& cfg, int H, int W);      // host logic only; a size no forward has: InvalidArgumentError
  // nullptr where this handle can add residuals, else why not (split CFG on, a dtype mode without a test); host logic only
  const char* residuals_refused() const;
  // forward_nchw with residuals given by the caller: all skip_shapes tensors back to back, NCHW fp32 (device) -> staging buffers in the stream dtype,
  // attached until clear_residuals / forward_nchw; residuals == nullptr: detached.  Refusals (InvalidArgumentError) come before any launch.
  void forward_residuals_nchw(const float* x, const int* timesteps, const float* context, int n_ctx, const float* label, int B, int H, int W,
                              const float* residuals, float scale, float* out, hipStream_t s);
  void clear_residuals();
  bool has_residuals() const { return res_key_ != 0; }
  // A control net is this class in control mode: the embeddings, input entries and middle block through the same loaders, run_entry, set_context and
  // K / V caches, no decoder; every entry's output (entry 0: + the hint features, the residual input of its convolution) goes through its 1x1
  // convolution into a residual buffer that persists for the plan.  forward() then leaves the skip_shapes tensors in control_residuals().
  UNet(const ControlCfg& cfg, int compute_dt, int stream_dt, WeightSource& src, hipStream_t st);
  bool is_control() const { return control_; }
  const ControlCfg& control_cfg() const { return ccfg_; }
  // the hint embedder, once per hint: hint NCHW fp32 [n][hint_in][8H][8W] (device) -> features NHWC [B][H*W][mc] in the stream dtype for the plan
  // (B, H, W); entry n + b of a batch B = 2n (the CFG pair) uses the hint of entry b.  Never per step.
  void set_hint(const float* hint, int n, int B, int H, int W, hipStream_t s);
  const void* hint_features() const { return hint_g_; }
  const std::vector<void*>& control_residuals() const { return ctl_res_; }
  // reference-shaped entries: hint -> features NCHW fp32 [n][mc][H][W]; the whole control forward -> all residual tensors back to back, NCHW fp32
  void embed_hint_nchw(const float* hint, int n, int H, int W, float* out, hipStream_t s);
  void control_forward_nchw(const float* x, const int* timesteps, const float* context, int n_ctx, const float* label, const float* hint, int B, int H, int W,
                            float* residuals_out, hipStream_t s);
  void* unet_in(int B, int H, int W);     // ensures the plan exists
  float* eps_out() { return eps_; }
  int compute_dt() const { return cdt_; }
  int mix_classes() const { return mix_; }     // MixClass bits in force (a SDXL_DTYPE_F32_SPLIT_MIX_F16W model on parameters that are not f16 values falls back to F32_SPLIT_MIX's)
  // dtype of the NHWC input the sampler writes (unet_in) and of the attention operands: the compute dtype, except that the
  // split-operand mode (DT_HL GEMM operands) keeps the 4-channel input and q / k / V^T in plain fp32
  int input_dt() const { return cdt_ == DT_HL ? DT_F32 : cdt_; }
  int attn_dt() const { return cdt_ == DT_HL ? DT_F32 : cdt_; }
  void set_use_graph(bool g) { use_graph_ = g; }
  // per-handle option: run the two entries of a batch-2 forward (the CFG pair) as two concurrent batch-1 chains on two
  // streams, the second released after `release_offset` GEMM launches of the first; bit-identical results
  void set_split_cfg(bool on, int release_offset) {
    if (on && res_key_) throw InvalidArgumentError("set_split_cfg: split CFG cannot be combined with attached skip residuals (ControlNet); detach them first");
    split_cfg_ = on; split_offset_ = release_offset;
  }
  void set_fused_cross_attention(bool on) { fuse_xattn_ = on; }
  void set_gn_from_producer(bool on) { gn_from_producer_ = on; }   // re-plans (arena + graph) on the next forward, like the two options above
  // one eager forward of the current plan/context with hipEvents around every launch, summed per kernel class
  void profile(int B, int H, int W, float ms[Profiler::NCLS], int launches[Profiler::NCLS], double flops[Profiler::NCLS],
               hipStream_t s);
  float eager_ms(int B, int H, int W, hipStream_t s);     // the chain profile() runs, without the per-launch events (best of three)
  size_t weight_bytes() const { return warena_.off; }
  void* weight_base() const { return warena_.base; }
  // weight_bytes() of a model with these MixClass bits in force, from the layout pass alone (no device call, no source)
  static size_t weight_layout_bytes(const UNetCfg& cfg, int compute_dt, int stream_dt, int mix);

 private:
  UNet(const UNetCfg& cfg, int compute_dt, int stream_dt, int mix);      // everything but the weights
  // build_weights: plans (+ the f16-exactness guard on the source), then load_weights twice -- over a dry arena and an empty source to size the
  // reservation (layout_weights), then for real
  void build_weights(WeightSource& src, hipStream_t st);
  std::vector<StPlan> plan_transformers(const std::vector<ParamSpec>& specs, std::vector<std::string>* f16_names) const;
  size_t layout_weights(const std::vector<ParamSpec>& specs, const std::vector<StPlan>& plans);
  void load_weights(WeightBuilder& wb, const std::vector<StPlan>& plans);
  void ensure_plan(int B, int H, int W);
  void run(Exec& ex, const float* t_dev, int t_stride, int b0, int nb);
  struct Skips { std::vector<Act> cat; std::vector<int> cx, hs_h, hs_w; };      // concat buffers, the column where each one's skip half starts, resolution after every input entry
  void alloc_skips(Exec& ex, int B, int H, int W, Skips& k);
  // the body of one plan entry (run's loops, run_block); add: a tensor of dst's shape added to the output of a Conv entry (a control net's hint features)
  void run_entry(Exec& ex, int section, int index, const Act& src, const Act& dst, int B, int h, int w, int si, const Act* add = nullptr);
  const float* res_block(Exec& ex, const ResBlockW& w, const Act& x, int B, int H, int W, const Act& out, float* out_gn_part = nullptr);
  void spatial_transformer(Exec& ex, const STW& w, int st_index, const Act& x, int B, int H, int W);

  UNetCfg cfg_;
  int cdt_, sdt_;
  int mix_ = 0;                          // MixClass bits (split-operand engine): classes on plain f16 operands
  bool mix_knob_ = false;                // the bits came from sdxl_debug_set "mix_classes" (no f16-exactness fallback)
  bool mix_mode_ = false;                // the handle was created in a SDXL_DTYPE_F32_SPLIT_MIX* / _F16W mode, whatever the fallback left in mix_
  bool attn16_ = false;                  // some transformer runs its self-attention on the f16 kernels (key-split workspace)
  DeviceArena warena_;
  std::vector<BlockW> inp_, out_;
  BlockW mid_res1_, mid_res2_;   // middle_block: res1 -> transformer (in mid_res1_.st) -> res2
  Lin lin1_t_, lin2_t_, lin1_l_, lin2_l_, embcat_;
  NormW norm_out_; Lin conv_out_;
  int emb_total_ = 0;
  // cross-attention K / V^T caches (one per transformer block, in execution order)
  struct KV { void* k = nullptr; void* vt = nullptr; void* xa = nullptr; void* xa_lo = nullptr; };   // xa: operand-order image for the fused epilogue (f16; with xa_lo: hi / lo halves of the fp32-class projection)
  std::vector<std::vector<KV>> kv_;     // [spatial transformer][block]
  std::vector<const STW*> st_list_;
  DeviceArena ctx_arena_;
  int ctx_B_ = 0, n_ctx_ = 0, vt_ld_ctx_ = 0;
  bool ctx_xa_ = false;      // set_context packed the operand-order context image (kv_[..].xa) for this n_ctx_
  float* label_emb_ = nullptr;           // [B][4mc]
  bool label_valid_ = false;             // the last set_context computed label_emb_ (run_block sets the context without a label)
  // plan
  int pB_ = 0, pH_ = 0, pW_ = 0;
  DeviceArena act_;
  void* in_ = nullptr; float* eps_ = nullptr;
  float *temb_ = nullptr, *g1_ = nullptr, *emb_ = nullptr, *ebias_ = nullptr, *gn_partial_ = nullptr, *tconv_ = nullptr;
  // split-K workspaces of the implicit GEMM (slabs + arrival counters), one per concurrent chain
  float* skws_[2] = {nullptr, nullptr}; unsigned* skcnt_[2] = {nullptr, nullptr}; size_t skws_bytes_ = 0;
  bool fuse_ln_ = false;                 // f16 compute + f16 residual stream: LayerNorms are folded into the GEMMs
  bool use_graph_ = true;
  // split-CFG mode: the two entries of a batch-2 forward run as two independent batch-1 chains on two streams (fork / join
  // by events, captured into the same graph); the second chain has its own scratch arena
  bool split_cfg_ = false; int split_offset_ = 0;
  bool plan_split_ = false; int graph_off_ = 0;
  bool fuse_xattn_ = true, plan_xattn_ = true;   // cross-attention inside the query projection's epilogue (f16 engines)
  WarmSeq warm_;                    // weight warming schedule of the current plan (recorded on its first forward)
  float* attn_xws_[2] = {nullptr, nullptr}; unsigned* attn_xcnt_[2] = {nullptr, nullptr};   // cross-workgroup key split: per chain (split-CFG runs two)
  bool graph_warm_ = false;         // the captured graph carries the warming workgroups
  size_t attn_xcnt_bytes_ = 0;
  int demote_mask_ = 0, graph_demote_ = 0;                 // hl_demote classes in force since the last set_context / captured in the graph
  std::vector<std::pair<float*, float>> demote_flags_;      // (device address of a packed matrix's exact-f16 flag, its packed value) per class bit, filled lazily
  std::vector<int> demote_flag_cls_;
  void apply_demote_weights(hipStream_t s);
  bool gn_from_producer_ = true, plan_gn_ = true;   // GroupNorm statistics from the producing convolution's epilogue where its kernel can (f16); part of the plan key
  hipStream_t s2_ = nullptr; hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
  DeviceArena act2_;
  hipGraphExec_t graph_ = nullptr;
  const float* graph_t_ = nullptr; int graph_ts_ = 0; int plan_runs_ = 0;
  // skip residuals: sources (dense NHWC rows in the stream dtype, one per skip_shapes entry) for the plan res_B_ x res_H_ x res_W_, the segment table
  // run's one launch walks and the scale it reads, both in device memory.  res_key_: 0 = none attached, else a number that changes whenever the set of
  // sources does -- part of the graph key (graph_res_key_), so attaching and detaching re-capture and a new scale or new values do not.
  void stage_residuals(const float* residuals, int B, int H, int W, float scale, hipStream_t s);
  void prepare_residuals();      // (re)builds the table for the current plan's concat buffers; outside any capture
  int res_key_ = 0, res_serial_ = 0, graph_res_key_ = 0;
  int res_B_ = 0, res_H_ = 0, res_W_ = 0;
  DeviceArena res_arena_;
  std::vector<const void*> res_src_;
  SkipSeg* res_table_ = nullptr; float* res_scale_ = nullptr;
  int res_segs_ = 0; unsigned long long res_chunks_ = 0; bool res_table_ok_ = false;
  const void* res_dst_mid_ = nullptr;      // the table's last destination: run checks that its concat buffers are where the table says
  // control mode
  bool control_ = false;
  ControlCfg ccfg_;
  Lin hint_conv_[8]; std::vector<Lin> zero_; Lin mid_out_;
  void run_control(Exec& ex, int B, int H, int W, void* in);
  std::vector<void*> ctl_res_;             // persistent residual buffers of the plan (dense NHWC, stream dtype), skip_shapes order; zero-filled with the plan
  std::vector<size_t> ctl_res_bytes_;
  DeviceArena hint_arena_;
  void* hint_g_ = nullptr; int hint_n_ = 0, hint_B_ = 0, hint_H_ = 0, hint_W_ = 0;
  const void* graph_hint_ = nullptr;
};

// ------------------------------------------------------------------------------------------ VAE
struct VaeResW { NormW n1, n2; Lin c1, c2, nin; bool has_nin = false; int cin = 0, cout = 0; };
struct VaeMidW { VaeResW b1, b2; NormW an; Lin q, k, v, proj; int C = 0; };
// The two blocks of the autoencoder that exist as single-op entries too (sdxl_vae_res_block / sdxl_vae_attn_block): free functions over a WeightBuilder and an
// Exec, so that the entries run the code Vae runs.  vae_load_res: p.norm1 / conv1 / norm2 / conv2 (+ p.nin_shortcut where the parameters have one);
// vae_load_attn: p.norm / q / k / v / proj_out into m (m.C set by the caller).  vae_res_block: ResnetBlock::forward x -> out; vae_attn_block:
// ConvSelfAttentionBlock::forward in place on the stream tensor y (the f16 C = 512 flash kernel, else QK^T GEMM -> row softmax -> P V GEMM in query passes).
VaeResW vae_load_res(WeightBuilder& wb, const std::string& p, int cin, int cout);
void vae_load_attn(WeightBuilder& wb, const std::string& p, VaeMidW& m);
void vae_res_block(Exec& ex, const VaeResW& w, const Act& x, int B, int H, int W, const Act& out, int n_group);
void vae_attn_block(Exec& ex, const VaeMidW& w, const Act& y, int B, int H, int W, int n_group);

class Vae {
 public:
  Vae(const VaeCfg& cfg, int compute_dt, WeightSource* dec_src, WeightSource* enc_src, hipStream_t st);
  ~Vae();
  const VaeCfg& cfg() const { return cfg_; }
  // LatentDecoder::decode_latent (stablediffusion/mod.rs:263-266): latent NCHW fp32 [n,4,h,w] -> NHWC image [n][8h*8w][3]
  // (fp32, internal buffer); returns the buffer
  const float* decode(const float* latent_nchw, int n, int h, int w, hipStream_t s);
  void decode_nchw(const float* latent_nchw, int n, int h, int w, float* out_nchw, hipStream_t s);
  void latent_to_image(const float* latent_nchw, int n, int h, int w, unsigned char* out_hwc, hipStream_t s);
  // LatentDecoder::encode_image / image_to_latent (:239-261): -> latent NCHW fp32 [n,4,H/8,W/8]
  void encode_nchw(const float* img_nchw, int n, int H, int W, float* latent_out, hipStream_t s);
  void image_to_latent(const unsigned char* img_hwc, int n, int H, int W, float* latent_out, hipStream_t s);
  size_t weight_bytes() const { return warena_.off; }
  void* weight_base() const { return warena_.base; }
  static size_t weight_layout_bytes(const VaeCfg& cfg, int compute_dt, bool decoder, bool encoder);      // weight_bytes() from the layout pass alone (no device call)

 private:
  Vae(const VaeCfg& cfg, int compute_dt) : cfg_(cfg), cdt_(compute_dt) {}
  // the loader: decoder and / or encoder (null: left out) into `arena`; run over a dry arena and empty sources first to size the reservation
  void load_weights(DeviceArena& arena, WeightSource* dec_src, WeightSource* enc_src, hipStream_t st);
  void res_block(Exec& ex, const VaeResW& w, const Act& x, int B, int H, int W, const Act& out);
  void mid(Exec& ex, const VaeMidW& w, const Act& x, int B, int H, int W);
  void run_decode(Exec& ex, const Act& in, int n, int h, int w, const Act& out);
  void run_encode(Exec& ex, const Act& in, int n, int H, int W, const Act& out);
  VaeMidW load_mid(WeightBuilder& wb, const std::string& p, int c);

  VaeCfg cfg_;
  int cdt_;
  DeviceArena warena_;
  bool has_dec_ = false, has_enc_ = false;
  // decoder
  Lin post_quant_, d_conv_in_, d_conv_out_; NormW d_norm_out_; VaeMidW d_mid_;
  // up_fold: the upsampler runs on its folded phase matrices (Lin::w_fold) -- the general three-MFMA form only: a layer whose parameters are all single f16
  // values keeps the 3x3 weights and their two-MFMA form.  -1 = not read yet (the flag lives in the arena: replicas know it after the broadcast)
  struct DecBlk { VaeResW r[3]; Lin up; bool has_up = false; int up_fold = -1; };
  std::vector<DecBlk> d_blocks_;
  // encoder
  Lin quant_, e_conv_in_, e_conv_out_; NormW e_norm_out_; VaeMidW e_mid_;
  struct EncBlk { VaeResW r[2]; Lin down; bool has_down = false; };
  std::vector<EncBlk> e_blocks_;
  DeviceArena act_;
  size_t act_peak_ = 0;
  float* gn_workspace(Exec& ex, int n);
  // dtype of the residual stream and of the 3- / 4- / 8-channel ends: the compute dtype, except that the split-operand mode
  // (DT_HL operands for the GEMMs) keeps them in plain fp32
  int io_dt() const { return cdt_ == DT_HL ? DT_F32 : cdt_; }
};

// ------------------------------------------------------------------------------------------ CLIP text encoder (Embedder)
struct ClipBlockW { NormW attn_ln, mlp_ln; Lin qkv, out, fc1, fc2; };

// CLIP<B> of the reference (clip/mod.rs:62-151): token + position embedding, n_layer pre-LN causal transformer blocks,
// final LayerNorm + eot pooling + text projection.  Runs once per prompt (Embedder::text_to_conditioning,
// stablediffusion/mod.rs:661-770), so it is launch/weight-bandwidth bound: the weights are streamed once per call.
class ClipText {
 public:
  ClipText(const ClipCfg& cfg, int compute_dt, int stream_dt, WeightSource& src, hipStream_t st);
  ~ClipText();
  void set_use_graph(bool g) { use_graph_ = g; }
  const ClipCfg& cfg() const { return cfg_; }
  // CLIP::forward_hidden (:94-112): ids int32 device [B][S] -> out fp32 device [B][S][n_state], the residual stream after
  // the first hidden_idx blocks (no final LayerNorm)
  void forward_hidden(const int* ids, int B, int S, int hidden_idx, float* out, hipStream_t s);
  // CLIP::forward_hidden_pooled (:114-151): hidden = input of block hidden_idx; pooled fp32 [B][embed_dim] =
  // LayerNorm(last)[argmax ids] . text_projection
  void forward_hidden_pooled(const int* ids, int B, int S, int hidden_idx, float* hidden, float* pooled, hipStream_t s);
  size_t weight_bytes() const { return warena_.off; }
  void* weight_base() const { return warena_.base; }
  static size_t weight_layout_bytes(const ClipCfg& cfg, int compute_dt);      // weight_bytes() from the layout pass alone (no device call)

 private:
  ClipText(const ClipCfg& cfg, int compute_dt, int stream_dt);
  void load_weights(DeviceArena& arena, WeightSource& src, hipStream_t st);      // run over a dry arena and an empty source first to size the reservation
  void run(const int* ids, int B, int S, int n_blocks, int tap, float* hidden, float* pooled, hipStream_t s);
  void block(Exec& ex, const ClipBlockW& w, const Act& x, int B, int S, const Act& ln, const Act& qk, void* vt, int npad,
             const Act& ao, const Act& h);
  ClipCfg cfg_;
  int cdt_, sdt_;
  DeviceArena warena_, act_;
  const void* tok_ = nullptr; const void* pos_ = nullptr;
  std::vector<ClipBlockW> blocks_;
  NormW final_ln_; Lin proj_;
  float* mask_ = nullptr;                    // causal mask [S][S] (lives in act_)
  hipGraphExec_t graph_ = nullptr; long key_[6] = {0, 0, 0, 0, 0, 0}; int runs_ = 0; bool use_graph_ = true;
};

// ------------------------------------------------------------------------------------------ sampler
// mirrors Conditioning<B> (stablediffusion/mod.rs:544-555); all device fp32
struct Conditioning {
  const float* unconditional_context_full = nullptr;        // [77][ctx_full]
  const float* unconditional_context_open_clip = nullptr;   // [77][1280]
  const float* context_full = nullptr;                      // [n][77][ctx_full]
  const float* context_open_clip = nullptr;                 // [n][77][1280]
  const float* unconditional_channel_context = nullptr;     // [adm]
  const float* unconditional_channel_context_refiner = nullptr;
  const float* channel_context = nullptr;                   // [n][adm]
  const float* channel_context_refiner = nullptr;
  int n = 1, n_ctx = 77, height = 1024, width = 1024;
};

#ifdef SDXL_MEASURE
extern bool g_debug_no_cfg;   // sdxl_debug_set("no_cfg"): base model without the unconditional branch (changes the semantics:
                              // measurement builds only)
#endif

// sdxl_guidance of the public header: how the two branches of an iteration become e (formulas there)
constexpr int kGuidanceCfg = 0, kGuidanceOff = 1;
struct Guidance {
  int mode = kGuidanceCfg;
  float rescale = 0.f;
  int n_scales = 0;
  float scales[kMaxSeeds] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int t_lo = 0, t_hi = 0x7fffffff;
  bool plain() const { return mode == kGuidanceCfg && rescale == 0.f && n_scales == 0 && t_lo == 0 && t_hi == 0x7fffffff; }
};

// sdxl_control of the public header: how a control net's residuals enter a trajectory, as a scale per iteration and batch entry
struct Control {
  float scale = 1.f;
  int n_scales = 0;
  float scales[kMaxSeeds] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int t_lo = 0, t_hi = 0x7fffffff;
  int cond_only = 0;
};
// host logic only: the first complaint about `c` (`single`: one branch, no CFG pair), nullptr where it is valid
const char* control_error(const Control& c, bool single);
// host logic only: the scales of one control net over a trajectory, out[iters + 1][8]:  out[i][b] = s(i, b) of the public header for the iteration at
// timesteps[i] and batch entry b of B = n (single) or 2 n, 0 for b >= B; row `iters` is zeros (where a device step index rests after the last
// iteration).  nullptr, or the complaint: control_error, n outside the batch, n_scales neither 0 nor n, a null pointer.
const char* control_scale_table(const Control& c, int n, bool single, const int* timesteps, int iters, float* out);

// The noise levels of one trajectory: iteration i runs at alphas_cumprod a[i] and lands on ap(i) = a[i + 1], a_end behind the last
// entry (1: the complete trajectory, the data itself).  t[i] is what the UNet is fed (rounded to float), what the guidance interval compares and
// what LCM scales; an integer list has t[i] = ts[i], a[i] = alphas[ts[i]]; a sigma list a[i] = 1 / (1 + sigma_i^2) and t[i] = sigma_to_t(sigma_i).
// t_end: the training timestep behind the last entry of an integer list (-1: none; TCD reads it), meaningless where from_sigmas.
struct Schedule {
  std::vector<double> t, a;
  double a_end = 1.0;
  int t_end = -1;
  bool from_sigmas = false;
  size_t size() const { return a.size(); }
  bool empty() const { return a.empty(); }
  double ap(size_t i) const { return i + 1 < a.size() ? a[i + 1] : a_end; }
};
constexpr int kSigmasRoundT = 1;      // SDXL_SIGMAS_ROUND_T
constexpr int kRowCols = 5;           // (c_x, c_0, c_1, c_2, c_z) per iteration

// The trajectory minus the UNet: the coefficient table, the guidance interval and the launches between two UNet forwards.  Diffuser::diffuse
// drives one with the UNet's output; sdxl_sampler_step_replay (the op-level test seam) drives one with given noise predictions.
struct StepIo {                       // device buffers of one trajectory (seeds: host array [n], nullptr = explicit noise)
  float* latent = nullptr;            // [n][4][HW] fp32, updated in place
  int eps_ld = 4;                     // row stride of the noise predictions handed to after_forward
  void* unet_in = nullptr; int in_dt = DT_F32; int in_ld = 4;     // next UNet input NHWC [B][HW][in_ld], B = n (single) or 2n
  const float* reference = nullptr; const unsigned char* mask = nullptr; const float* step_noise = nullptr;
  const uint64_t* seeds = nullptr;
};
class StepLoop {
 public:
  StepLoop();
  ~StepLoop();
  StepLoop(const StepLoop&) = delete;
  StepLoop& operator=(const StepLoop&) = delete;
  // Builds the StepCoef table (host f64 -> f32) and the active-iteration array of one trajectory, uploads them and runs the do_update = 0
  // launch: *step_idx = 0, the step-0 inpainting blend, the first UNet input and timestep.  `single`: one branch, no CFG (B = n).  Returns the
  // number of iterations.  alphas: the n_train alphas_cumprod values as f64 (TCD reads them).  sc: the schedule -- the only source of an
  // iteration's (t, a, ap) (Diffuser::schedule_of_timesteps on Diffuser::step_schedule for the reference's rule).
  // prediction: kPredictionEpsilon or kPredictionV, what the rows handed to after_forward mean.  A schedule Diffuser::schedule_error refuses
  // (alphas_cumprod == 0 at an iteration's timestep under kPredictionEpsilon) throws InvalidArgumentError before anything is launched, and so
  // does a table with c_z != 0 where io.seeds == nullptr (Diffuser::explicit_noise_error).  kSolverLcm / kSolverTcd allocate no history, kSolverDpmpp2M one,
  // kSolverDpmpp3M two.  The order of a multistep solver starts at one: whatever the history buffers hold is not read on iteration 0.
  int begin(const std::vector<double>& alphas, const Schedule& sc, int solver, double eta, double cfg_scale, const Guidance& g,
            bool single, int n, int HW, const StepIo& io, hipStream_t s, int prediction = kPredictionEpsilon);
  // behind the UNet forward of iteration i: eps [B][HW][eps_ld] fp32 (cond entries first) -> the CFG rescale factors where rescale is on and
  // the iteration active, then the update + advance launches
  void after_forward(int i, const float* eps, hipStream_t s);
  float* t_dev() const { return t_dev_; }       // device scalar: the timestep of the next UNet call
  const float* hist() const { return hist_; }   // kSolverDpmpp2M / kSolverDpmpp3M: x0 of the previous iteration [n][4][HW]
  const float* hist2() const { return hist2_; } // kSolverDpmpp3M: the x0 before that one

 private:
  StepCoef* table_ = nullptr; int table_cap_ = 0;
  // the per-iteration active flags next to the table (uploaded where an interval leaves an iteration out), the CFG rescale partials and the n factors
  int* active_ = nullptr; int active_cap_ = 0;
  float* moments_ = nullptr; size_t moments_cap_ = 0;
  float* factors_ = nullptr;
  int* step_idx_ = nullptr; float* t_dev_ = nullptr;
  float* hist_ = nullptr; size_t hist_cap_ = 0;
  float* hist2_ = nullptr; size_t hist2_cap_ = 0;
  // the trajectory begin() set up
  StepParams p_{};
  float rescale_ = 0.f;
  std::vector<int> act_;           // host copy of the active flags: which iterations run the rescale launches
};

class Diffuser {
 public:
  Diffuser(const UNetCfg& cfg, int compute_dt, int stream_dt, WeightSource& src, const float* alphas_host, int n_train,
           hipStream_t st, int mix = 0);
  ~Diffuser();
  UNet& unet() { return *unet_; }
  // Diffuser::sample_latent (stablediffusion/mod.rs:317-332); noise0 plays gen_noise(); out: NCHW fp32 [n,4,h/8,w/8]
  void sample_latent(const Conditioning& c, double cfg_scale, int n_steps, const float* noise0, float* out, hipStream_t s);
  // Diffuser::sample_latent_with_inpainting (:334-353, :434-483); mask u8 (1 = keep generated), step_noise [iters][n,4,h,w]
  void sample_latent_inpaint(const Conditioning& c, double cfg_scale, int n_steps, const float* reference,
                             const unsigned char* mask, const float* noise0, const float* step_noise, float* out,
                             hipStream_t s);
  // Diffuser::refine_latent (:355-376)
  void refine_latent(const float* latent, const Conditioning& c, double cfg_scale, int step_start, int n_steps,
                     const float* noise, float* out, hipStream_t s);
  // the same three calls with the noise drawn on the device from one 64-bit seed per batch entry (host array [n]) and the
  // gen_noise() * sigma term of :427 live: sigma_t = eta sqrt((1 - ap) / (1 - a)) sqrt(1 - a / ap), eta in [0, 1]
  void sample_latent_seeded(const Conditioning& c, double cfg_scale, int n_steps, const uint64_t* seeds, double eta, float* out,
                            hipStream_t s);
  void sample_latent_inpaint_seeded(const Conditioning& c, double cfg_scale, int n_steps, const float* reference,
                                    const unsigned char* mask, const uint64_t* seeds, double eta, float* out, hipStream_t s);
  void refine_latent_seeded(const float* latent, const Conditioning& c, double cfg_scale, int step_start, int n_steps,
                            const uint64_t* seeds, double eta, float* out, hipStream_t s);
  static std::vector<int> step_schedule(int n_steps, int step_start, int n_train);
  // host logic only: the first complaint about a caller's list (n outside 1..n_train, a value outside 0..n_train-1, not strictly decreasing;
  // every message names "timesteps"), nullptr where it is valid
  static const char* timesteps_error(const int* ts, int n, int n_train);
  // a per-handle list that replaces step_schedule in all six trajectory calls (n == 0 or nullptr: back to the reference's rule).  A list
  // timesteps_error refuses throws InvalidArgumentError and the handle keeps what it had.  With a list the calls' n_steps must equal its length,
  // step_start must be 0 for sampling and inpainting, and refine_latent needs ts[0] == n_train - step_start - 1 (InvalidArgumentError otherwise).
  // t_end: the training timestep the last iteration lands on, ap = alphas[t_end] there (-1: ap = 1, the complete trajectory); it must lie in
  // -1 .. ts[n - 1] - 1 (timesteps_end_error names "timesteps").  Setting a timestep list (or clearing it) drops the handle's sigma list.
  static const char* timesteps_end_error(const int* ts, int n, int t_end, int n_train);
  void set_timesteps(const int* ts, int n, int t_end = -1);
  // the handle's timestep list; empty: the reference's rule -- and while a sigma list is set, which is then the list in force
  const std::vector<int>& timesteps() const { static const std::vector<int> none; return sigmas_.empty() ? timesteps_ : none; }
  int timesteps_end() const { return timesteps_end_; }
  // Noise-level (sigma) lists, k-diffusion's sigma = sqrt((1 - a) / a).  sigmas_error: host logic only -- the first complaint (n
  // outside 1..n_train, a value that is not finite and > 0, not strictly decreasing, sigma_end outside [0, sigmas[n - 1]), unknown flags, a table
  // of fewer than two entries; every message names "sigmas"), nullptr where the list is valid.  set_sigmas: the list every following
  // trajectory runs, with sigma_end behind the last entry (0: the complete trajectory); n == 0 or nullptr drops it, and the handle is back on
  // the timestep list or rule it had before.  While it is set it is the only list in force.
  static const char* sigmas_error(const double* sigmas, int n, double sigma_end, int flags, int n_train);
  void set_sigmas(const double* sigmas, int n, double sigma_end, int flags);
  const std::vector<double>& sigmas() const { return sigmas_; }
  double sigma_end() const { return sigma_end_; }
  int sigma_flags() const { return sigma_flags_; }
  // k-diffusion's sigma_to_t in f64 on L_j = 0.5 ln((1 - alphas[j]) / alphas[j]): low the largest j <= n_train - 2 with L_j <= ln sigma (0 if
  // none), w = clamp((L_low - ln sigma) / (L_low - L_{low+1}), 0, 1), t = (1 - w) low + w (low + 1); kSigmasRoundT: rint(t), ties to even
  static double sigma_to_t(const double* alphas, int n_train, double sigma, int flags);
  // the two ways to a Schedule; both require a list their *_error accepts (InvalidArgumentError otherwise)
  static Schedule schedule_of_timesteps(const double* alphas, int n_train, const int* ts, int n, int t_end = -1);
  static Schedule schedule_of_sigmas(const double* alphas, int n_train, const double* sigmas, int n, double sigma_end, int flags);
  // sdxl_continue_latent: the handle's list from a given latent.  renoise == false: the latent as it is (noise ignored); else the start is
  // sqrt(a_0) latent + sqrt(1 - a_0) z, z = noise or the kDrawInitial draw of seeds (exactly one of the two).  A multistep solver starts first order.
  void continue_latent(const float* latent, const Conditioning& c, double cfg_scale, int n_steps, const float* noise, const uint64_t* seeds,
                       double eta, bool renoise, float* out, hipStream_t s);
  // (c_x, c_0, c_1, c_2, c_z) of x' = c_x x + c_0 x0 + c_1 x0p + c_2 x0pp + c_z z per entry of the schedule, f64, out[kRowCols * i ..] (host logic only;
  // formulas in include/sdxl_mi355.h, sdxl_solver_coefficients).  kSolverDpmpp2M: what diffuse() rounds into its table.  kSolverDdim: the
  // DDIM update folded into the same four numbers.  alphas: n_train values in (0, 1).  The rows do not depend on the prediction type; it
  // decides only whether a == 0 at an iteration's timestep (zero terminal SNR) is admitted: kPredictionV writes that row as the limit
  // lambda -> -inf, kPredictionEpsilon throws InvalidArgumentError.  kSolverLcm (eta must be 0) and kSolverTcd (eta is gamma):
  // the first-order rows (c_x, c_0, 0, 0, c_z) of include/sdxl_mi355.h, finite at a == 0 as written; TCD reads alphas at
  // floor((1 - gamma) t') and so needs training timesteps: on a sigma list it throws InvalidArgumentError (the message names "sigmas").
  // kSolverDpmpp3M: the only solver with c_2 != 0.
  static void solver_coefficients(const double* alphas, int n_train, const Schedule& sc, int solver, double eta, double* out,
                                  int prediction = kPredictionEpsilon);
  // host logic only: why a trajectory of `solver` on ts cannot run on explicit noise (its eta == 0 table has a c_z != 0, and explicit noise
  // carries no tensor for that term), nullptr where it can: DDIM, 2M, TCD (gamma = 0 there) and a one-entry LCM list
  static const char* explicit_noise_error(const double* alphas, int n_train, const Schedule& sc, int solver, int prediction);
  // host logic only: the first complaint about the (a, ap) pairs of the schedule under `prediction`, nullptr where the trajectory can run.
  // kPredictionEpsilon: a == 0 on an iteration (x0 would divide by it) -- the message names v-prediction.  kPredictionV: a outside [0, 1)
  // or ap outside (0, 1].
  static const char* schedule_error(const Schedule& sc, int prediction);
  // kPredictionEpsilon (default) or kPredictionV: what the UNet's output means to every following trajectory of this handle
  void set_prediction(int prediction);
  int prediction() const { return prediction_; }
  // kSolverDdim (default), kSolverDpmpp2M, kSolverDpmpp3M, kSolverLcm or kSolverTcd: the update every following trajectory of this handle runs
  void set_solver(int solver);
  int solver() const { return solver_; }
  // guidance options, a per-handle choice like the solver.  guidance_error: host logic only -- the first complaint about `g` (for a refiner
  // handle: anything but the default or kGuidanceOff), nullptr where it is valid.  set_guidance requires a valid `g`.  Guidance{} is
  // the call's scalar as every entry's scale on every iteration (the reference's line); kGuidanceOff runs the conditional branch alone (batch n).
  static const char* guidance_error(const Guidance& g, bool is_refiner);
  void set_guidance(const Guidance& g);
  const Guidance& guidance() const { return guidance_; }
  bool is_refiner() const { return is_refiner_; }
  std::vector<float> step_ms;   // per-iteration GPU time of the last trajectory (hipEvent), for "UNet step ms p50"
  bool time_steps = false;
  // parity instrumentation: after DDIM iteration i the latent [n,4,h,w] is copied to trace + i * numel (device, caller-owned)
  // for i < trace_cap -- the per-step latents the oracle's `trace` lists hold (drift reports, tests)
  float* trace = nullptr; int trace_cap = 0;

 private:
  // what the six public calls share: latent_ sized, its start (noise, the seeded fill, or `renoise` re-noised to step_start), diffuse, copy out
  struct Trajectory {
    const float* noise = nullptr;                             // explicit start (or re-noise) tensor; nullptr with seeds
    const float* renoise = nullptr; int step_start = 0;       // refine_latent: the finished latent and where to re-noise it to
    const float* start = nullptr;                             // continue_latent: the start latent as it is; with renoise0: re-noised to the list's a_0
    bool renoise0 = false;
    const float* reference = nullptr; const unsigned char* mask = nullptr; const float* step_noise = nullptr;      // inpainting
    const uint64_t* seeds = nullptr; double eta = 0.0;        // seeded noise
  };
  void trajectory(const Conditioning& c, double cfg_scale, int n_steps, const Trajectory& t, float* out, hipStream_t s);
  // context setup, then StepLoop::begin and one UNet forward + StepLoop::after_forward per iteration
  // the list of this call: the handle's own (checked against n_steps and step_start as set_timesteps documents) or step_schedule
  Schedule call_schedule(int n_steps, int step_start, bool renoise, bool listed_only = false) const;
  void diffuse(float* latent, const Conditioning& c, const Schedule& sc, double cfg_scale, const float* reference,
               const unsigned char* mask, const float* step_noise, hipStream_t s, const uint64_t* seeds = nullptr, double eta = 0.0);
  std::unique_ptr<UNet> unet_;
  std::vector<double> alphas_;
  int n_train_;
  bool is_refiner_;
  // device state
  float* latent_ = nullptr; size_t latent_cap_ = 0;
  float* noise_ = nullptr; size_t noise_cap_ = 0;     // re-noise tensor of refine_latent_seeded
  int solver_ = kSolverDdim;
  std::vector<int> timesteps_;                        // empty: step_schedule
  int timesteps_end_ = -1;
  std::vector<double> sigmas_;                        // non-empty: the list in force (timesteps_ rests)
  double sigma_end_ = 0.0; int sigma_flags_ = 0;
  int prediction_ = kPredictionEpsilon;
  Guidance guidance_;
  StepLoop loop_;
  float* ctx_buf_ = nullptr; size_t ctx_cap_ = 0;     // [2n][77][ctx] cond then uncond
  float* y_buf_ = nullptr; size_t y_cap_ = 0;
  const void* cached_ctx_key_[4] = {nullptr, nullptr, nullptr, nullptr}; int cached_n_ = 0;
};

}  // namespace sdxl
