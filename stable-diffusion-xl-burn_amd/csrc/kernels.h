// Kernel launch interface of the MI355X (gfx950) SDXL engine.  Everything here is device-side HIP written
// for CDNA4 (64-lane wavefronts, MFMA, LDS); the host engine (unet.cpp / vae.cpp / sampler.cpp) only calls
// these launchers.  Layout convention everywhere: activations are NHWC / token-major [rows][channels] with
// an explicit row stride ("ld", in elements), so a tensor can live inside a wider (concat) buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdexcept>

namespace sdxl {

// compute precision of a model instance
// DT_HL: split-operand storage "HL16" (igemm_common.h): a logical fp32 value as two f16 numbers (hi, lo), 4 bytes per element,
// every 16 channels = 32 halfs [16 hi | 16 lo] -- operands of the 3-MFMA fp32-class GEMM the VAE runs at the reference's precision
enum DType : int { DT_F32 = 0, DT_F16 = 1, DT_HL = 2 };

static inline size_t dt_size(int dt) { return dt == DT_F16 ? 2 : 4; }

// ---------------------------------------------------------------------------------------------------------
// Implicit GEMM:  C[M,N] = gather(A)[M,K] * Wp[N,K]^T   (conv3x3 / conv1x1 / linear; NHWC; K = taps*Cin)
// Replaces burn Conv2d / nn::Linear call sites (reference unet/mod.rs:116-120,1036-1053,729-731,765-770,
// 793,801,903,929,975-984,1041; autoencoder/mod.rs:161-180,281-283,461-472,526-529).
struct IgemmParams {
  const void* A;        // source activations [B][Hin][Win] rows of lda elements (dtype a_dt)
  const void* W;        // packed weights [Npad][Kpad] in compute dtype, K order = (tap, cin), zero padded
  const void* Wf;       // optional: the same f16 weights in MFMA fragment order (launch_repack_wfrag) -- linear layers / 1x1 convs the
                        // weights-in-registers kernel may take (igemm_wreg.hip); null = not packed that way
  int a_dt;             // dtype of A in memory (DT_F16 / DT_F32); converted to compute dtype while staging
  int B, Hin, Win, Cin, lda;
  int Hout, Wout;       // M = B*Hout*Wout
  int ksize, stride, pad, up;   // up=1: nearest-2x upsample of the source fused into the gather
  int M, N, K, Kpad;    // N = logical packed columns (<= Npad)
  // epilogue:  v = acc + bias[n] + ebias[b*ebias_ld + n];  act;  + R;  store
  const float* bias;    // [Npad] fp32 (packed order) or null
  const float* ebias;   // [B][ebias_ld] fp32 or null (ResBlock time-embedding add, unet/mod.rs:1092)
  int ebias_ld;
  int rpb;              // rows per batch element (Hout*Wout or tokens) for ebias / transposed store
  int act;              // 0 none, 1 GEGLU: packed column pairs (x,gate) in 16-wide groups -> x*gelu_erf(gate);
                        // 2 GELU(erf), 3 QuickGELU x*sigmoid(1.702x)  (CLIP MLP, clip/mod.rs:296-320; generic kernel only)
  const void* R; int ldr; int r_dt;     // residual added after act (same logical shape as output)
  void* C; int ldc; int c_dt;           // output for columns n < n_split (after GEGLU: n/2)
  int n_split;          // columns >= n_split go to the transposed output (set = N when unused)
  void* Ct; int ct_rows; int ct_ld;     // Ct[b][n - n_split][key]  (ct_rows rows per batch, row stride ct_ld), dtype c_dt
  // LayerNorm folded into the GEMM (reference layernorm/mod.rs:34-49 followed by nn::Linear): A holds the RAW rows x,
  // W holds diag(gamma) W, bias holds beta W + b, and the epilogue applies  v = rstd[m]*acc - rstd[m]*mu[m]*ln_cs[n] + bias[n]
  // with (mu, rstd) from the partial row sums the PRODUCER of x left behind: ln_stat[slot][m] = (mean, M2 = sum (x - mean)^2) over the
  // 64 columns of slot, ln_slots = K/64 slots per row, summed here in slot order (deterministic).  null -> plain GEMM.
  const float* ln_stat; int ln_slots; const float* ln_cs; float ln_invc; float ln_eps;
  const float* ln_eps_ptr;   // optional device scalar overriding ln_eps
  // when set, the staged epilogue stores (mean, M2) -- shifted sums, no sum x^2 - (sum x)^2 -- of every 64-column group of the stored output rows into
  // stat_out[n/64][m] (plain stores, every entry written once) -- the statistics of the LayerNorm that reads this output
  float* stat_out; int stat_slots;
  // split-K workspace (optional): fp32 partial slabs [tile][slice][256 x 128] + one arrival counter per tile (zero between
  // launches: the last-arriving slice re-arms it).  splitk is filled by the launcher (igemm_splitk_slices); 0 / 1 = off.
  float* splitk_ws; size_t splitk_ws_bytes; unsigned* splitk_cnt; int splitk;
  // cross-attention fused into this (query) projection: when xa_k is set the epilogue replaces the q tile by
  // softmax(q K_h^T * xa_scale) V_h per 64-column head before the store (igemm_glds.hip xattn_inplace).  xa_k = the context
  // keys / values of the batch entries in MFMA operand order (launch_xattn_pack); batch entry of a row = m / rpb.
  const void* xa_k; int xa_nctx; float xa_scale;
  // split-precision form (round 6): xa_k holds the HI halves f16(x) of the context keys / values and xa_k_lo the LO halves f16(x - hi), both in the
  // operand order of launch_xattn_pack; the epilogue then splits q and P the same way and runs three MFMAs per product (Kh qh + Kh ql + Kl qh, likewise
  // V^T P^T): the arithmetic of attn_d64_hl_kernel inside the projection's epilogue.  null = plain f16 attention.  One-MFMA-row wave tiles only.
  const void* xa_k_lo;
  // GroupNorm statistics of the stored output, from the epilogue (256x128 kernel; igemm_gn_part_ok): gn_part[M/256][N] (mean, M2)
  // of every column over the 256 rows of a tile -- the consumer's GroupNorm merges row tiles and channels (norm.hip, chan_part)
  float* gn_part;
  const float* acc_scale;   /* [0] = 1 / weight scale, [1] != 0: every packed weight is exactly one f16 (lo halves all zero) */  // DT_HL compute: the packed weights carry a power-of-two factor (exact); device scalar 1 / factor the epilogue multiplies the
                           // accumulators by (lives in the weight arena, so replicas that receive the arena by broadcast need no host copy); null = 1
  const float* a_scale;     // DT_HL compute: 2^-e of an A operand converted by launch_f32_to_hl_scaled (null = 1); exact.  One value per batch entry:
  int a_scale_rpb;          // output rows per entry of a_scale (row m reads a_scale[m / a_scale_rpb]); 0 = one value for all rows
  int hl_wexact_ok; // A/B knob (sdxl_debug_set "hl_weights_exact", default 1): split-operand launches may leave out the w_lo MFMAs when acc_scale[1] says every weight is one f16
  int xa_vec64;     // measure builds (sdxl_debug_set "xa_vec64"): the fused cross-attention epilogue reads its per-column vectors with the original 64-lane
  // weight warming (round 4): the launch also brings `warm_bytes` of the weights a LATER GEMM of the same stream will read into the
  // memory-side Infinity Cache -- spare workgroups behind the tile grid (kernels whose grid leaves CUs idle: igemm_wreg_selected) do
  // nothing but read them.  No effect on any result; null = off.
  const void* warm[3]; unsigned warm_bytes[3];     // up to three regions (filled from the front)
  int splitk_wt;    // split-K slabs published by write-through stores instead of plain stores + release fence (set by the launcher from the A/B knob "splitk_wt", default 1)
                    // VMEM loads instead of the scalar cache -- the hazard experiment of DESIGN 9.2 / 10.4
  int wreg_xcd2d;   // A/B knob (sdxl_debug_set "wreg_xcd2d"): weights-in-registers kernel, XCDs own 2-D patches of tiles (half the column tiles x ~ a quarter of
                    // the row tiles each) instead of whole row-tile runs -- fewer unique operand bytes per XCD's L2; set by the launcher
  int epi_staged;   // A/B knob (sdxl_debug_set "igemm_epilogue_staged"): 1 = LDS-staged epilogue everywhere, 0 = direct row-per-lane where it applies
  // f16 SHADOW of an fp32 residual stream (round 6; weights-in-registers kernel only, igemm_wreg_selected): next to the fp32 rows C the epilogue stores
  // shadow[m][n] = f16(value * shadow_gamma[n]) -- the A operand of the GEMM behind the NEXT LayerNorm (gamma = that norm's), whose weights stay
  // un-folded: LN(x) W + b = rstd (x o gamma) W - rstd mu (gamma W) + (beta W + b).  With stat_out (the fp32 rows' statistics) the LayerNorm launch
  // between two GEMMs of a split-operand transformer block disappears.  null = off.
  void* shadow; int shadow_ld; const float* shadow_gamma;
  float shadow_lo_scale;    // > 0: the shadow row is [hi (N columns) | lo (N columns)], lo = f16((value * gamma - hi) * shadow_lo_scale): the (hi, lo) A operand of a GEMM packed (w | w / scale).
                            // < 0: the shadow is an HL16 tensor (shadow_ld in LOGICAL elements, un-scaled lo halves): read as an f16 row of 2 N columns by a GEMM whose weight is
                            // packed twice in the HL16 interleave (launch_pack_linear_hilo mode 2)
  // Nearest-2x upsample + 3x3 convolution as FOUR 2x2-tap convolutions on the source (upsample_fold.h), one launch: the rows are ordered
  // [phase = 2a + b][entry][i][j] (M = 4 ph_rows), ph_rows = B * Hin * Win rows per phase, a multiple of the tile's rows so that a row tile lies in one
  // phase.  Geometry of ONE phase: ksize = 2, stride = 1, up = 0, Hout = Hin, Wout = Win; tap (dy, dx) of row (i, j) reads source pixel
  // (i + dy - pad + a, j + dx - pad + b) with pad = 1 -- a pad that differs per phase and axis; pixels outside the source come from the zero page.
  // Phase ph multiplies the weights at W + ph * ph_wbytes ([Npad][Kpad] each, K = 4 Cin) and its row (entry, i, j) is stored to output row
  // (entry * 2 Hin + 2 i + a) * 2 Win + 2 j + b.  Plain epilogue only (bias, accumulator scales; no residual / statistics / split output).
  // Pipe kernels on f16 and split-operand elements (igemm_glds.hip); 0 = off: every other kernel ignores the fields, the selection refuses them.
  int ph_rows; unsigned ph_wbytes;
};
// ---- kernel selection (select.cpp: host-only, no HIP call).  Knobs that influence WHICH kernel runs, written by sdxl_debug_set and
// snapshotted once per launch; zero_page is an input of the same kind, filled by the launcher (the DMA kernels' zero page exists on this device)
struct SelectKnobs {
  int igemm_variant = 0;    // test hook: -1 generic kernel only, 0 auto, > 0 a forced tile number -- one the shape refuses falls back to auto
  int igemm_wreg = 1;       // 0 = the auto selection never picks the weights-in-registers kernel
  int wreg_xattn = 1;       // 0 = the fused cross-attention stays on the pipe kernels
  int hl_tile96 = 29;       // split-operand GEMMs.  bit 0: 96x128 for linears, bit 1: ... for 3x3 convs too (not selected), bit 2: 4-wave 128x160 for N % 160 == 0, N % 128 != 0
                            // layers, bit 3: ... wherever the cost model prefers it, bit 4: in-launch split-K for the K >= 10240 convolutions
  int igemm_tsw = 1;        // 0 = the V^T part of a fused QKV projection keeps the LDS-staged transposed epilogue (no operand-swapped k-loop)
  int igemm_unrolled = 1;   // measure builds: 0 = auto selection on the rolled pipelined kernels
  int wide_db = 0;          // measure builds: 1 = the wide GEGLU kernel with register-double-buffered fragments
  int attn_variant = 0;     // -1: generic kernel only, 0: auto, 2: 32x32x16 deferred-max kernel, 6: key-split kernel, 7 / 8: mix level 0 / 1, 9: auto without mixing
  int attn_xsplit = 1;      // 0 = never pick the cross-workgroup key split (mix level 2)
  int zero_page = 0;        // not a knob: the launcher's "zero page present"
};
bool select_knob_set(const char* key, int value);   // false: not a selection knob
SelectKnobs select_knobs_snapshot();                // (zero_page = 0: the launcher fills it)
enum IgemmFamily : int { IG_NONE = 0, IG_GLDS = 1, IG_PIPE = 2, IG_WIDE = 3, IG_WREG = 4, IG_GENERIC = 5, IG_MEASURE = 6 };
// what launch_igemm launches: the kernel family and its template arguments, the grid and the dynamic LDS bytes
struct IgemmChoice {
  int family;               // IgemmFamily; IG_NONE: empty output, nothing to launch; IG_MEASURE: `measure` goes to launch_igemm_measure
  int bm, bn, ns;           // tile rows / columns, ring depth (IG_WREG: prefetch depth L)
  int wgm, nw;              // waves along M, waves
  int elem, a_elem;         // compute element (DT_F16 / DT_F32 / DT_HL); IG_GENERIC: element of A in memory
  int xa, xh, tsw, s2;      // fused cross-attention (IG_WREG: the context's 96-key blocks, 1 .. 4; else 0 / 1), its split-precision form, operand-swapped V^T epilogue, one rendezvous per two k-tiles
  int splitk;               // k-slices per tile (1 = off)
  int mode, db, measure;    // measure builds: knock-out mode of the weights-in-registers kernel, double-buffered wide kernel, measure-only variant number
  int grid, block, lds;
};
IgemmChoice igemm_select(const IgemmParams& p, int compute_dt, const SelectKnobs& k);
// the same rules for run_conv, which promises its consumers a statistics buffer / a shadow and budgets weight warming BEFORE the launch
// (on the snapshot it then launches with: igemm_launch_knobs)
bool igemm_gn_part_ok(const IgemmParams& p, const SelectKnobs& k);
bool igemm_wreg_selected(const IgemmParams& p, const SelectKnobs& k);         // the auto selection would run this launch on the weights-in-registers kernel
bool igemm_wreg_xattn_selected(const IgemmParams& p, const SelectKnobs& k);   // ... a fused query projection + cross-attention (xa_k, f16 form)
// launches the fused cross-attention epilogue takes (f16 operands, head dim 64); otherwise run the projection and the attention kernel separately.
// n_ctx <= 96: every form -- the pipe kernels' epilogue (xattn_inplace), its split-precision twin (xattn_inplace_hl) and the weights-in-registers XA
// instantiation; a function of the shape alone.  96 < n_ctx <= 384 (two to four 77-token chunks): the weights-in-registers XA instantiation alone, which
// walks the context in 96-key blocks (xattn_unit_long); true only where the selection will run that form -- `wreg_form`: the launch carries fragment-order
// weights and the plain f16 context image (no xa_k_lo); `k`: the knobs it will be launched with.  The pipe and split-precision forms keep their 96-key
// limit and the un-fused fallback above it.  The ONE predicate of the plan (UNet::set_context, spatial_transformer), run_conv, the single-op entry and
// the selection (wreg_takes).
constexpr int xattn_long_max_blocks = 4;      // 96-key blocks the long form is selected for (the kernel has no limit of its own)
bool igemm_xattn_ok(int a_dt, int c_dt, int M, int N, int K, int rpb, int n_ctx, const SelectKnobs& k, bool wreg_form);
// the phase form of an upsample convolution (IgemmParams::ph_rows, filled): the selection has a pipe tile for it.  Asked by run_conv before it
// hands the launch the folded weights; false: the layer keeps the gather form.  A function of one entry's shape (rows per phase and entry, N, K).
bool igemm_phase_ok(const IgemmParams& p, int compute_dt, const SelectKnobs& k);
// K [B][n_ctx][C], V^T [B][C][vt_ld] (f16) -> operand-order image of xattn_pack_bytes(B, C, n_ctx) bytes (once per prompt): per (entry, head)
// ceil(n_ctx / 96) blocks of 24 fragments -- up to 96 keys one block, the bytes and layout the pipe epilogues read
size_t xattn_pack_bytes(int B, int C, int n_ctx);
void launch_xattn_pack(const void* K, const void* Vt, void* out, int B, int C, int n_ctx, int vt_ld, hipStream_t s);
int igemm_splitk_slices(const IgemmParams& p);                       // 1 or 3: depends on one batch entry's shape only
size_t igemm_splitk_ws_bytes(int batch, int rows_per_entry, int n_max);   // slab bytes a plan must provide
constexpr int kSplitkCounters = 4096;                                // arrival counters a plan must provide (zeroed once)
SelectKnobs igemm_launch_knobs();      // the process's knobs + the current device's zero page (igemm.hip)
void launch_igemm(const IgemmParams& p, int compute_dt, const SelectKnobs& knobs, hipStream_t s);
void launch_igemm(const IgemmParams& p, int compute_dt, hipStream_t s);      // ... on a snapshot of its own
// [Npad][Kpad] f16 row-major packed weights -> fragment order (same bytes): per 32-row block and 64-deep k-tile four 1-KiB MFMA
// A-operand fragments, contiguous over k -- what igemm_wreg_kernel streams straight into registers.  Npad % 32 == 0, Kpad % 64 == 0.
void launch_repack_wfrag(const void* w, void* wf, int Npad, int Kpad, hipStream_t s);
void igemm_set_warm(int v);      // A/B knob (sdxl_debug_set "igemm_warm"): 0 = no weight warming workgroups; read when a UNet plan records its GEMM sequence
int igemm_warm_enabled();
void igemm_set_splitk_wt(int v);
void igemm_set_wreg_xcd2d(int v);
void igemm_set_hl_weights_exact(int v); // A/B: 0 keeps all three MFMAs per product even where the packed weights are exact f16 values
void igemm_set_xa_vec64(int v);          // measure builds: see IgemmParams::xa_vec64
void igemm_set_epilogue_staged(int v);   // A/B: 1 forces the LDS-staged epilogue (default 0: direct row-per-lane epilogue on whole wave tiles)
#ifdef SDXL_MEASURE
void igemm_set_timeline(void* device_buf);
void igemm_set_wreg_timeline(void* device_buf);   // igemm_wreg.hip: [workgroups][8 waves][16] coarse stamps
void igemm_set_wide_timeline(void* device_buf);   // igemm_glds.hip: [workgroups][8 waves][8] coarse stamps of the wide (GEGLU) kernel   // igemm_measure.hip: stamp buffer of the timeline kernel variants
int igemm_timeline_words();
#endif
// the dynamic-LDS limit of a kernel (up to 160 KiB), raised once per (kernel, device); dev = the current device, < kMaxDevices
constexpr int kMaxDevices = 64;
template <auto Kernel> inline void set_max_dynamic_lds(size_t lds, int dev) {
  static bool done[kMaxDevices] = {};
  if (done[dev]) return;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    throw std::runtime_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  done[dev] = true;
}
// per-device state owned by igemm_glds.hip
const void* igemm_zero_page();          // null until igemm_glds_init() ran on the current device
int igemm_current_device();
void igemm_glds_init();          // allocates the zero page the DMA fast paths read from: halo pixels of the convolutions, key-tail rows of the attention kernels (call once per process)

// per-entry scale workspace of launch_f32_to_hl_scaled (declared further down)
constexpr int kHlAbsBlocks = 128;
static inline size_t hl_scale_floats(int nb) { return (size_t)nb * (kHlAbsBlocks + 1); }
static inline float* hl_scale_inv(float* scale_io, int nb) { return scale_io + (size_t)nb * kHlAbsBlocks; }

// ---------------------------------------------------------------------------------------------------------
// GroupNorm (32 groups, NHWC) -- reference groupnorm/mod.rs:52-82 (+ SiLU silu.rs:14-16)
struct GroupNormParams {
  const void* X; int x_dt; int ldx;    // [B][HW] rows, C channels
  void* Y; int y_dt; int ldy;
  const float* gamma; const float* beta;
  float* partial;      // workspace: groupnorm_workspace_floats(B, G) floats
  int B, HW, C, G;
  float eps;
  const float* eps_ptr; // optional device scalar overriding eps (per-norm eps stored with the weights)
  int silu;            // fuse x*sigmoid(x) after the affine
  int nsplit;          // filled by the launcher helper
  // statistics left by the PRODUCER of X (IgemmParams::gn_part): chan_part[B][chan_rt][C] (mean, M2) over chan_rows rows each;
  // when set, no statistics kernel runs -- the apply kernel merges row tiles and channels in its prologue
  const float* chan_part; int chan_rt; int chan_rows;
  // optional side output of the statistics pass (fp32 input only): per batch entry kHlAbsBlocks block maxima of |x| -- the partials
  // launch_f32_to_hl_scaled's conversion kernel reduces (the statistics pass reads the whole tensor anyway: a split-operand skip convolution of the
  // same ResBlock input then needs no absmax pass).  Layout [B][kHlAbsBlocks]; slots beyond the row splits are written as zeros.
  float* absmax_out;
};
int  groupnorm_nsplit(int B, int HW, int C);
// workspace of launch_groupnorm for B batch entries (a run over entries [b0, b0+nb) of a larger plan may use the slice at
// b0 * groupnorm_workspace_floats(1, G)): per (entry, group) kGnMaxSplit row-split partials (count, mean, M2) + (mean, rstd)
constexpr int kGnMaxSplit = 128;
static inline size_t groupnorm_workspace_floats(int B, int G) { return (size_t)B * G * (kGnMaxSplit * 3 + 2); }
void launch_groupnorm(const GroupNormParams& p, hipStream_t s);

// LayerNorm over the last dim -- reference layernorm/mod.rs:34-49
struct LayerNormParams {
  const void* X; int x_dt; int ldx;
  void* Y; int y_dt; int ldy;
  const float* gamma; const float* beta;
  int rows, C; float eps;
  const float* eps_ptr;   // optional device scalar overriding eps
  float dup_scale;        // f16 output only, != 0: the row is written twice.  > 0: y[0, C) = f16(LN(x)) and y[C, 2C) = that f16 value * dup_scale (a power of two) --
                          // the A operand of a GEMM whose weights are packed as (hi | lo / dup_scale) halves along K (launch_pack_linear_hilo mode 0).
                          // < 0: y[C, 2C) = f16((LN(x) - hi) * |dup_scale|), the LO half of the activation -- against weights packed as (w | w / |dup_scale|) (mode 1)
};
void launch_layernorm(const LayerNormParams& p, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------
// Fused attention softmax(Q K^T * scale) V, head dim 64 -- reference backend.rs:88-128 (Backend::qkv_attention)
struct AttnParams {
  const void* Q; int ldq;      // [B][Nq] rows, head h at columns h*64..
  const void* K; int ldk;      // [B][Nk] rows
  const void* Vt; int vt_ld;   // V transposed: [B][H*64][vt_ld], keys contiguous, zero beyond Nk
  void* O; int ldo;
  int dt;                      // dtype of Q,K,Vt,O (compute dtype)
  int B, H, Nq, Nk;
  float scale;                 // 1/sqrt(d)
  const float* mask; int ldmask;   // optional additive [Nq][Nk] fp32 (0 / -inf), null in UNet/VAE
  int q_dt = 0;                // split-operand kernel only: DT_F32 (0) or DT_HL -- Q rows in HL16 (ldq in logical elements)
  int o_dt = 0;                // split-operand kernel only: DT_F32 (0), DT_HL -- O written as HL16 rows (ldo in logical elements), the next GEMM's operand -- or DT_F16 (rounded once: an f16 out-projection's operand)
  // key halves on DIFFERENT workgroups (attn_d64_mix_kernel level 2, round 4): workspace of attention_xsplit_ws_bytes(B, H, Nq) bytes and
  // attention_xsplit_counters(B, H, Nq) zero-initialised tickets (they re-arm themselves); null = that form is never picked
  float* xws = nullptr; unsigned* xcnt = nullptr;
  int demote = 0;              // split-operand kernel only (precision-frontier instrument): lo halves of Q and P dropped -- with K / V^T lo halves zeroed
                               // by the caller the kernel computes the f16 flash kernel's products (f16 q, k, v, p; fp32 accumulation)
};
size_t attention_xsplit_ws_bytes(int B, int H, int Nq);
size_t attention_xsplit_counters(int B, int H, int Nq);
enum AttnKernel : int { AT_GENERIC = 0, AT_F16 = 1, AT_V2 = 2, AT_KS = 3, AT_MIX = 4 };   // (5 stays unused: it named the software-pipelined kernel in recorded choices)
// what launch_attention_d64 launches
struct AttnChoice {
  int kernel;               // AttnKernel: generic (elem DT_F16 / DT_F32), DMA-staged 16x16x32, 32x32x16 deferred-max (ns ring slots), key-split, mixed block sizes
  int mix, big_heads;       // AT_MIX: level 0 / 1 / 2 (-1 otherwise) and the heads that run in the large blocks
  int ns, elem, ko;         // (ko: measure builds, knock-out bits of the key-split body)
  int grid_x, grid_y, block, lds;
};
AttnChoice attn_select(const AttnParams& p, const SelectKnobs& k);
void launch_attention_d64(const AttnParams& p, hipStream_t s);
// split-operand (fp32-class) head-dim-64 attention: Q / O fp32 (ldq / ldo in floats), K [B][Nk] rows and Vt [B][H*64][vt_ld] rows in
// HL16 (ldk / vt_ld in LOGICAL elements: a row is 2 * ld halfs), no mask; vt_ld a multiple of 64 keys, zero beyond Nk.  Returns false
// when the shape / alignment needs launch_attention_d64 on fp32 tensors.
bool launch_attention_d64_hl(const AttnParams& p, hipStream_t s);
// the same contraction for ONE wide head of 512 channels (VAE mid block): flash kernel, scores never materialised; Q/K/O rows
// hold the heads at columns h*512, Vt is [B][H*512][vt_ld] with zero columns up to a multiple of 32 keys.  f16, no mask;
// returns false when the shape / alignment needs the unfused path.  p.scale = d^-1/2.
bool launch_attention_hd512(const AttnParams& p, hipStream_t s);
#ifdef SDXL_MEASURE
void attention_set_timeline(void* device_buf);   // [workgroups][4 waves][8] coarse stamps of the key-split attention body
#endif

// row softmax for the unfused attention path (VAE mid block, d=512, 1 head): P[r][:] = softmax(S[r][:]*scale + mask)
// S fp32 [rows][lds] (scores from igemm), P in dtype p_dt [rows][ldp]; columns n..npad-1 of P are zero filled.
void launch_softmax_rows(const float* S, int lds, void* P, int p_dt, int ldp, int rows, int n, int npad, float scale,
                         const float* mask, int ldmask, int mask_rows, hipStream_t s, float p_scale = 1.0f, float* p_scale_out = nullptr);
// p_scale / p_scale_out: P is stored times the power of two p_scale and {1 / p_scale, 0} is left at p_scale_out -- the accumulator scale
// (IgemmParams::acc_scale layout) of the split-operand P V product that consumes it

// ---------------------------------------------------------------------------------------------------------
// Small-M linear (GEMV): Y[b][n] = act_in(X[b][:]) . Wp[n][:] + bias[n]   (time/label/emb MLPs, M<=8)
struct GemvParams {
  const float* X; int ldx;     // fp32 [Bm][K]
  const void* W; int w_dt; int Kpad;   // packed [N][Kpad]
  const float* bias;           // fp32 or null
  float* Y; int ldy;           // fp32 [Bm][N]
  const float* Yadd;           // optional fp32 [Bm][N] added to the result (t_emb + label_emb)
  int Bm, N, K;
  int silu_in;                 // apply SiLU to X while loading
  int silu_out;                // apply SiLU to the result
};
void launch_gemv(const GemvParams& p, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------
// elementwise / layout
// sinusoidal embedding (unet/mod.rs:21-39): out[b][0:half]=cos(t*f), [half:]=sin(t*f); t read from device
void launch_timestep_embedding(const float* t_dev, int t_stride, float* out, int Bm, int dim, hipStream_t s);
// NCHW fp32 -> NHWC (dtype dt), optional batch replication (src batch stride 0)
void launch_nchw_to_nhwc(const float* src, int src_batch_stride, void* dst, int dt, int B, int C, int HW, int ldd,
                         float scale, hipStream_t s);
void launch_nhwc_to_nchw(const void* src, int dt, int lds, float* dst, int B, int C, int HW, float scale, hipStream_t s);
// generic cast copy rows: dst[r][c] = src[r][c]
void launch_copy_rows(const void* src, int sdt, int lds, void* dst, int ddt, int ldd, int rows, int C, hipStream_t s);
void launch_fill_zero(void* p, size_t bytes, hipStream_t s);
// fp32 rows -> split-operand HL16 rows (C % 16 == 0, row strides in logical elements, dst stride % 16 == 0)
// exact[0] = 1.0f if every x * wscale of src[0..n) is exactly one f16 value (the packed lo halves are all zero), else 0.0f;
// `accumulate`: AND with the value already there (several tensors of one fused matrix)
void launch_f16_exact(const float* src, size_t n, float wscale, float* exact, hipStream_t s, bool accumulate = false);
void launch_f32_to_hl(const void* src, int lds, void* dst, int ldd, size_t rows, int C, hipStream_t s);
// the same for a tensor whose range the model does not bound (residual stream, VAE hidden state): converted times the power of two
// that brings max|x| into [2^13, 2^14) -- PER BATCH ENTRY (nb entries of rows / nb rows each: an entry's bits never depend on its batch
// neighbours).  scale_io: hl_scale_floats(nb) device floats -- [nb][kHlAbsBlocks] per-block max|x| partials (no atomics, no memset: every
// launch rewrites them), then the nb factors 2^-e at hl_scale_inv(scale_io, nb): pass that as IgemmParams::a_scale (a_scale_rpb = the GEMM's output rows per entry)
void launch_f32_to_hl_scaled(const void* src, int lds, void* dst, int ldd, size_t rows, int C, float* scale_io, hipStream_t s, int nb = 1,
                             bool have_partials = false);   // have_partials: a GroupNorm statistics pass over the same tensor left the maxima (GroupNormParams::absmax_out)
unsigned count_nonfinite(const void* src, int dt, int lds, size_t rows, int C, hipStream_t s);   // debugging aid (SDXL_NAN_CHECK): synchronises
void launch_f16_to_hl(const void* src, int lds, void* dst, int ldd, size_t rows, int C, hipStream_t s);   // f16 rows -> HL16 rows (lo = 0)
// fp32 rows -> two plain f16 row sets hi = f16(x), lo = f16(x - hi) (row stride ld16 each): the context images of the split-precision fused cross-attention
void launch_f32_to_f16_pair(const float* src, int lds, void* hi, void* lo, int ld16, size_t rows, int C, hipStream_t s);
void launch_hl_zero_lo(void* dst, int ldd, size_t rows, int C, hipStream_t s);   // HL16 rows: lo halves := 0 (precision-frontier instrument, UNet hl_demote)
void launch_round_f16(float* p, size_t n, hipStream_t s);   // p[i] = float(half(p[i])): parameters as a HalfPrecisionSettings record holds them
// create-time adapter merge: w[rows][cols] += scale * left[rows][rank] @ right[rank][cols], fp32 device tensors, in place.  Fixed arithmetic: per element
// acc = 0; acc = fmaf(left[r][j], right[j][c], acc) for j = 0 .. rank-1; w = fmaf(scale, acc, w).  scale == 0 launches nothing.
void launch_lora_merge(float* w, size_t rows, size_t cols, const float* left, const float* right, int rank, float scale, hipStream_t s);
void launch_i32_to_f32(const int* src, float* dst, int n, hipStream_t s);
// CLIP text encoder (clip/mod.rs:99-105,139-147): x[b][t][:] = tok[ids[b][t]][:] + pos[t][:] (tables in dtype w_dt);
// eot[b] = first index of max(ids[b][:]); sel[b][:] = x[b][eot[b]][:] as fp32; additive causal mask [n][n] (0 / -inf)
void launch_embed_tokens(const int* ids, const void* tok, const void* pos, int w_dt, void* x, int x_dt, int ldx, int B, int S,
                         int C, int n_vocab, hipStream_t s);
void launch_argmax_rows(const int* ids, int* out, int B, int S, hipStream_t s);
void launch_gather_rows(const void* x, int x_dt, int ldx, const int* idx, int S, float* out, int B, int C, hipStream_t s);
void launch_causal_mask(float* out, int n, hipStream_t s);
// conditioning_embedding (unet/mod.rs:41-57): out[n][E + w*dim] = [pooled | sinusoidal embedding of each of the w ints]
void launch_conditioning_embedding(const float* pooled, int E, const int* vals, int w, int dim, float* out, int n, hipStream_t s);

// Step table entry (host f64 -> f32): stablediffusion/mod.rs:407-428
// sigma: the DDIM eta term of :427 (0 on every explicit-noise trajectory; then sqrt_1map = sqrt(1 - ap), else sqrt(1 - ap - sigma^2))
// The DPM-Solver++(2M) table (kSolverDpmpp2M) is the second layout of the same 32 bytes: t, sqrt_a and sqrt_1ma as in the DDIM one
// (x0, the inpainting blend and ddim_advance_kernel read them alike), and the four coefficients of x' = c_x x + c_0 x0 + c_1 x0p + c_z z
// (include/sdxl_mi355.h, sdxl_solver_coefficients) where the DDIM layout keeps its three update terms and its padding.
struct StepCoef {
  float t; float sqrt_a; float sqrt_1ma;
  union { float sqrt_ap; float c_0; };
  union { float sqrt_1map; float c_x; };
  union { float pad; float c_2; };     // DDIM and 2M layouts: 0 (held the guidance scale until it became StepParams::scales); kSolverDpmpp3M: the
                                       // coefficient of the second history term
  union { float sigma; float c_z; };
  float c_1;     // padding of the DDIM layout (0)
};
static_assert(sizeof(StepCoef) == 32, "one table entry is eight floats in both layouts");
constexpr int kSolverDdim = 0, kSolverDpmpp2M = 1;   // SDXL_SOLVER_* of the public header
// the consistency solvers of the public header (few-step sampling): two host tables of first-order rows (c_x, c_0, 0, c_z) in the 2M
// layout, and one update text for both in the per-step kernel, StepParams::solver == kSolverRow1
constexpr int kSolverLcm = 3, kSolverTcd = 4;     // SDXL_SOLVER_LCM, SDXL_SOLVER_TCD (2 is no public solver)
constexpr int kSolverRow1 = 2;                     // kernel level only: never a handle's solver
// DPM++ 3M SDE: the 2M layout with one more history term, x' = c_x x + c_0 x0 + c_1 x0p + c_2 x0pp + c_z z, c_2 in StepCoef::c_2
constexpr int kSolverDpmpp3M = 5;                  // SDXL_SOLVER_DPMPP_3M
constexpr bool solver_is_row1(int solver) { return solver == kSolverLcm || solver == kSolverTcd; }
constexpr int kPredictionEpsilon = 0, kPredictionV = 1;   // SDXL_PREDICTION_* of the public header: what the UNet's output rows mean
// draw numbers of the seeded noise (counter word 1 of the generator); the public header carries the same values as SDXL_DRAW_*
constexpr uint32_t kDrawInitial = 0;
constexpr uint32_t draw_blend(uint32_t i) { return 1u + 2u * i; }
constexpr uint32_t draw_sigma(uint32_t i) { return 2u + 2u * i; }
constexpr int kMaxSeeds = 8;   // batch entries of one trajectory (Diffuser::diffuse: B <= 8)
struct DdimSeeds { uint64_t v[kMaxSeeds]; };   // per-entry seeds, passed by value in the kernel arguments
struct CfgScales { float v[kMaxSeeds]; };      // per-entry guidance scales, passed by value in the kernel arguments like the seeds
// The per-step kernel, one thread per latent pixel (step_kernel<SOLVER, SEEDED, PRED>, elementwise.hip, where every rounding is written out):
//   e  = ec                                  where !use_cfg, or on an inactive iteration (active != nullptr && !active[*step_idx]); eu is not read
//   e  = fma(ec - eu, scales[b], eu)         otherwise; times factors[b] where factors != nullptr (CFG rescale)
//   x0 = (x - e sqrt_1ma) / sqrt_a;  x = x0 sqrt_ap + e sqrt_1map (+ z sigma)   or, kSolverDpmpp2M,   x = c_x x + c_0 x0 + c_1 x0p (+ c_z z)
//   or, kSolverRow1,   x = c_x x + c_0 x0 (+ c_z z): the 2M line without its history term
//   or, kSolverDpmpp3M, x = c_x x + c_0 x0 + c_1 x0p + c_2 x0pp (+ c_z z): the 2M line with a second history term
// kPredictionV: the rows are v = alpha e - sigma x0, combined by the same two guidance lines (v, vc, vu for e, ec, eu), and then
//   x0 = x sqrt_a - v sqrt_1ma               no division: finite at sqrt_a == 0 (zero terminal SNR), where x0 = -v
//   e  = v sqrt_a + x sqrt_1ma               kSolverDdim only; the update lines behind x0 and e are those above
// then the inpainting blend for the next iteration and the refresh of the UNet input (NHWC, once per branch).
// eps: UNet output [Bu][HW][eps_ld] fp32-or-T rows; latent NCHW fp32 [n][4][HW].
struct StepParams {
  float* latent;             // [n][4][HW] fp32 NCHW (state)
  const void* eps; int eps_dt; int eps_ld;   // UNet output NHWC rows: cond batch entries [0,n), uncond [n,2n)
  const StepCoef* table; int* step_idx;
  int n, HW; int use_cfg;
  // guidance (include/sdxl_mi355.h, sdxl_guidance).  The default is the call's scalar in every scales[b], active = factors = nullptr.
  CfgScales scales;
  const int* active;         // device [iterations] or nullptr (every iteration active): 1 where guidance is on at that iteration's timestep
  const float* factors;      // device [n] or nullptr (no rescale): f_b of this iteration, left by launch_cfg_rescale_factors on the same stream
  // inpainting (optional): before the *next* UNet call latent = mask ? latent : ref*sqrt_a(next)+noise*sqrt_1ma(next)
  const float* ref; const unsigned char* mask; const float* step_noise; int n_steps_total;
  // seeded mode: the blend noise (draw_blend(next)) and the sigma noise (draw_sigma(idx)) are drawn in the thread from
  // seeds[b]; step_noise is not read.  seeded = 0 is the explicit-noise kernel, which never looks at sigma.
  int seeded; DdimSeeds seeds;
  void* unet_in; int in_dt; int in_ld; int in_rep;   // next UNet input NHWC [in_rep*n][HW][4]
  float* t_out;              // device scalar(s): timestep for the next UNet call
  // kSolverDpmpp2M: table holds the 2M layout and hist [n][4][HW] fp32 the x0 of the previous iteration (read where c_1 != 0, written by
  // every update); kSolverDdim reads neither.  kSolverRow1: the 2M layout with c_1 == 0; hist is neither read nor written (nullptr)
  // prediction: kPredictionEpsilon or kPredictionV (sits in the padding between solver and hist: no other member moves)
  int solver; int prediction; float* hist;
  // kSolverDpmpp3M: hist2 [n][4][HW] fp32 the x0 before hist's (read where c_2 != 0; receives hist's value wherever that was read, i.e. where
  // c_1 != 0: the shift happens per element inside the update, the two addresses never change).  Every other solver: nullptr, never looked at
  float* hist2;
};
// do_update=0: first call of a trajectory -- sets *step_idx = 0, applies the step-0 inpaint blend, writes the UNet
// input and timestep.  do_update=1: the update with table[*step_idx], blend for the next step, then advances.
void launch_step(const StepParams& p, int do_update, hipStream_t s);
// CFG rescale (Lin et al. 2023, section 3.4): factors[b] = fma(phi, sqrt(M2(ec_b) / M2(ecfg_b)), 1 - phi), M2 the centred sum of squares over the
// 4 * HW values of entry b, ecfg = fma(ec - eu, scales[b], eu); M2(ecfg_b) == 0 gives 1.  eps: rows [2n][HW][eps_ld] of eps_dt, cond entries
// first.  Two launches: per-block (count, mean, M2) partials, grid (cfg_moments_blocks(HW), n), then one block per entry that merges them in
// block-index order.  partials: device scratch of cfg_moments_floats(n, HW) floats.  No atomics: an entry's factor has the same bits alone and batched.
// The op sees the network's raw output rows whatever they mean: under kPredictionV the moments are those of vc and vcfg (what Lin et al. rescale).
constexpr int kCfgMomentsBlock = 256;
inline int cfg_moments_blocks(int HW) { return (HW + kCfgMomentsBlock - 1) / kCfgMomentsBlock; }
inline size_t cfg_moments_floats(int n, int HW) { return (size_t)n * cfg_moments_blocks(HW) * 6; }
void launch_cfg_rescale_factors(const void* eps, int eps_dt, int eps_ld, int n, int HW, const CfgScales& scales, float phi, float* partials,
                                float* factors, hipStream_t s);
// gen_noise (:378-388) with a seed: out [n][4][HW] fp32, entry b from seeds[b] (host array, n <= kMaxSeeds per launch), the
// same values the seeded per-step kernel draws in registers for (seed, hw, draw)
void launch_seeded_noise(float* out, const uint64_t* seeds, uint32_t draw, int n, int HW, hipStream_t s);
// noised = latent*sa + noise*sb   (refine_latent :363-367)
void launch_axpby(float* dst, const float* a, float sa, const float* b, float sb, size_t n, hipStream_t s);
// ControlNet skip residuals: ONE launch adds every residual tensor of a step into the tensor the decoder reads -- the skip halves of the
// concat buffers and the middle block's output.  A segment is `rows` rows of C channels: every src[k < K] dense [rows][C], dst rows of dst_ld elements,
// all in the dtype `dt` (DT_F32 / DT_F16) of the launch.  The table lives in device memory (fixed address: a captured graph keeps it), the scales too
// (changing them re-captures nothing).  `first` = 16-byte chunks of the segments before this one (filled by skip_table_check).  Segments must not
// overlap; the result does not depend on the grid.  Two ways to name the scales:
//   one scalar (step_idx_dev == nullptr, K == 1):  dst = round_to_dt(fma(*scales_dev, (float)src[0], (float)dst)), at every scale, 0 included;
//   a table (step_idx_dev != nullptr):  source k of a row has the scale s_k = scales_dev[(*step_idx_dev * K + k) * 8 + b], b = row / (rows / B) the
//     batch entry of the row -- a device table [iterations + 1][K][8] and the loop's device step index, so one captured launch serves every iteration.
//     Per element: v = (float)dst; for k = 0 .. K-1 in order, where s_k != 0: v = fmaf(s_k, (float)src[k], v); dst = round_to_dt(v) where any s_k != 0.
//     A source whose own scale is 0 is not read (it may hold NaN, or end before the chunk: a control net run on the conditional entries alone); a
//     chunk all of whose scales are 0 is not written.
constexpr int kSkipScaleEntries = 8;
constexpr int kSkipMaxSources = 4;
struct SkipSeg { void* dst; const void* src[kSkipMaxSources]; long long dst_ld; int rows; int C; unsigned long long first; };      // (src[k >= K] are not looked at)
// host logic only: nullptr where every segment can run -- dt is DT_F32 or DT_F16, K in 1..kSkipMaxSources, rows >= 0, C > 0, C % 8 == 0, dst_ld >= C,
// dst / every src[k < K] / the row pitch 16-byte aligned, fewer than 2^32 chunks; B == 0 is the one-scalar form, else B in 1..8 and every segment's
// rows a multiple of B --, else the complaint; fills SkipSeg::first and *total_chunks
const char* skip_table_check(SkipSeg* table_host, int n_seg, int K, int B, int dt, unsigned long long* total_chunks);
void launch_skip_add(const SkipSeg* table_dev, int n_seg, int K, unsigned long long total_chunks, const float* scales_dev, const int* step_idx_dev, int B,
                     int dt, hipStream_t s);
void launch_silu_inplace(void* p, int dt, size_t n, hipStream_t s);      // p[i] = silu(p[i]), dense, DT_F32 / DT_F16
// image post-process (stablediffusion/mod.rs:210-230): u8 = trunc(clamp(((x+1)/2)*255, 0, 255)), NHWC rows of 3
void launch_to_u8_image(const void* src, int dt, int lds, unsigned char* dst, size_t pixels, hipStream_t s);
// u8 HWC image -> NHWC activation (x/255)*2-1  (image_to_latent :239-255)
void launch_from_u8_image(const unsigned char* src, void* dst, int dt, int ldd, size_t pixels, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------
// weights: synthetic fill (bit-identical to oracle/config.py synth_values) and packing into device layouts
void launch_synth_fill(float* dst, size_t numel, uint64_t key, float scale, float mean, hipStream_t s);
// canonical Linear [K][N] fp32 (burn layout) -> packed [Npad][Kpad] (dt); optional GEGLU interleave
void launch_pack_linear(const float* src, void* dst, int dt, int K, int N, int Kpad, int Npad, int geglu,
                        int n_offset, hipStream_t s, const float* kscale = nullptr,    // kscale[k]: LayerNorm gamma fold
                        float wscale = 1.0f);                                          // power-of-two factor of the DT_HL packing
// the same packing with every weight as TWO f16 values along a doubled K: dst[n][k] = f16(w), dst[n][K + k] = f16((w - f16(w)) * lo_scale) -- against the A
// operand [a | a / lo_scale] (LayerNormParams::dup_scale) the f16 GEMM multiplies a by hi + lo: the weights are not rounded (22 significand bits), the
// activations once.  K % 32 == 0; Kpad = 2 K.
void launch_pack_linear_hilo(const float* src, void* dst, int K, int N, int Npad, int geglu, float lo_scale, hipStream_t s, int mode = 0, int n_offset = 0);   // n_offset: first packed row (fused matrices: Npad = this part's rows)
// mode 1: dst[n][K + k] = f16(f16(w) / lo_scale) -- the weight twice, for an A operand that carries (hi | lo * lo_scale) ACTIVATION halves (exact for f16-representable weights)
// mode 2: the weight twice in the HL16 INTERLEAVE -- dst[n][32 g + j] = dst[n][32 g + 16 + j] = f16(w[16 g + j]) (K % 16 == 0): an HL16 activation row of C logical channels IS an
//         f16 row of 2 C columns [16 hi | 16 lo | ...], so any f16 GEMM kernel multiplies (hi + lo) by w -- two MFMAs per product, exact for f16-representable weights
// LayerNorm fold helpers: column sums of the packed (rounded) weight rows; beta . W + bias in canonical column order
void launch_colsum_packed(const void* wp, int dt, int Kpad, int nrows, float* cs, hipStream_t s, const float* kscale = nullptr, int K = 0, int interleave = 0);   // kscale: cs[r] = sum_k kscale[k] packed[r][k]; interleave: the packed row holds the K weights twice in the HL16 interleave (first copies summed)
void launch_beta_dot(const float* w, const float* beta, const float* bias, float* out, int K, int N, hipStream_t s);
// canonical conv [Cout][Cin][kh][kw] fp32 -> packed [Npad][Kpad], k = (kh*kw_idx)*Cin + c
void launch_pack_conv(const float* src, void* dst, int dt, int Cout, int Cin, int ks, int Kpad, int Npad,
                      hipStream_t s, float wscale = 1.0f);   // wscale: power-of-two factor of the DT_HL packing (undone by IgemmParams::acc_scale)
// canonical 3x3 conv [Cout][Cin][3][3] fp32 -> [4][Cout][Cin][2][2]: the four 2x2-tap phase convolutions of a nearest-2x upsample in front of it
// (upsample_fold.h; fp32 sums in one fixed order); each phase then packs like any convolution (launch_pack_conv, ks = 2)
void launch_fold_upsample(const float* src, float* dst, int Cout, int Cin, hipStream_t s);
void launch_absmax(const float* src, size_t n, float* out_dev, hipStream_t s, bool accumulate = false);   // *out_dev = max(|src[i]|[, *out_dev])
// bias vector permuted the same way as GEGLU-packed columns (fp32 -> fp32)
void launch_pack_bias(const float* src, float* dst, int N, int Npad, int geglu, int n_offset, hipStream_t s);

}  // namespace sdxl
