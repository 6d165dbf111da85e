/* sdxl_mi355.h -- C ABI of the MI355X-native SDXL sampling engine (libsdxl_mi355.so).
 *
 * Drop-in boundary for the hot path of Gadersd/stable-diffusion-xl-burn: these are the entry points a Rust `cc` +
 * `bindgen` shim binds so that the reference's public model API keeps its signatures while all
 * arithmetic runs in hand-written HIP kernels for gfx950.  Each symbol cites the reference interface it replaces
 * (paths relative to the reference repository).
 *
 * Conventions
 *   - every tensor argument is a raw DEVICE pointer to contiguous fp32 data in the reference's own layout
 *     (NCHW images/latents, [B,N,C] tokens) unless stated otherwise; outputs go to caller-allocated device buffers;
 *   - `stream` is a hipStream_t passed as void*; NULL selects the context's own (blocking) stream.  A handle must only
 *     be used from one stream/thread at a time (the reference is single-threaded, src/bin/sample/main.rs:130-291);
 *   - every function returns 0 on success, non-zero on failure; sdxl_last_error() returns the thread-local message.
 *     Nothing aborts: the Rust shim maps non-zero to panic!/Err exactly where the reference asserts/unwraps
 *     (unet/mod.rs:73-76, :967-972; groupnorm/mod.rs:19-24);
 *   - weights are handed over as ONE flat fp32 buffer (host or device) holding the tensors listed by
 *     sdxl_*_param_spec() back to back, in that order, each in the reference's layout: nn::Linear [d_in,d_out],
 *     Conv2d [out,in,kh,kw], norm gamma/beta [C]  (python/save.py:20-25,56-72; src/model/load.rs:62-74,119-156).
 */
#ifndef SDXL_MI355_H
#define SDXL_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdxl_ctx sdxl_ctx;
typedef struct sdxl_unet sdxl_unet;
typedef struct sdxl_diffuser sdxl_diffuser;
typedef struct sdxl_vae sdxl_vae;
typedef struct sdxl_clip sdxl_clip;

enum { SDXL_OK = 0, SDXL_ERR_INVALID = 1, SDXL_ERR_RUNTIME = 2 };
/* precision of a model instance (measurements of every mode: DESIGN.md sections 4-6 and profiles/; the reference runs the UNet in f16 and the VAE in f32,
 * src/bin/sample/main.rs:121-122) */
enum {
  SDXL_DTYPE_F32 = 0,       /* strict parity: fp32 storage, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32); meets the unscaled 1e-3 on latents                       */
  SDXL_DTYPE_F16 = 1,       /* fp16 storage + fp16 MFMA operands, fp32 accumulation / statistics / softmax: the benchmarked mode                               */
  SDXL_DTYPE_F16_F32RES = 2,/* fp16 MFMA operands, fp32 residual stream                                                                                       */
  SDXL_DTYPE_F32_SPLIT = 3, /* fp32-class results on the f16 matrix pipe: fp32 stream, GEMM / attention operands as (hi, lo) f16 pairs, three MFMAs per product
                             * (two where every weight is an f16 value).  UNet / Diffuser, VAE, sdxl_conv2d, sdxl_linear, unmasked head-dim-64 sdxl_qkv_attention.
                             * Meets the unscaled 1e-3 on latents                                                                                             */
  SDXL_DTYPE_F32_SPLIT_MIX = 4, /* UNet / Diffuser only: F32_SPLIT with the self-attention and the GEGLU projection on plain f16 operands.  Inside the parity
                             * tests' SCALED 1e-3 bound on the 31-step and 100-step configurations, not below the unscaled 1e-3, over the scaled bound on
                             * the 4-step stress fixture                                                                                                       */
  SDXL_DTYPE_F32_SPLIT_MIX_F16W = 5, /* UNet / Diffuser only, for models whose PARAMETERS ARE f16 VALUES (what the reference's records hold, HalfPrecisionSettings:
                             * src/bin/sample/main.rs:37): F32_SPLIT_MIX + QKV projection, both out-projections, FF-out and the cross-attention query projection on
                             * plain f16 operands, LayerNorms folded through an f16 shadow of the stream.  Same limits as _MIX.  On other parameters the engine
                             * falls back to _MIX's classes (checked on the tensors at create time: sdxl_unet_mix_classes)                                     */
  SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2 = 6, /* _F16W with the class that carries most of its error at higher precision: the GEGLU projection's ACTIVATIONS as (hi, lo) f16
                             * pairs along a doubled K (two MFMAs per product on the same f16 kernel).  ~12 % slower than _F16W; inside the scaled bound on EVERY
                             * fixture of the parity tests, the 4-step inpainting stress fixture included.  Same f16-parameter requirement and fallback           */
  SDXL_DTYPE_F32_SPLIT_F16W = 7 /* UNet / Diffuser only: SDXL_DTYPE_F32_SPLIT for models whose PARAMETERS ARE f16 VALUES -- the same fp32-class arithmetic (two MFMAs per product,
                             * fp32 stream, split-operand attention; meets the unscaled 1e-3) with the transformer's linear layers on the F16 kernels: an HL16
                             * activation row is read as an f16 row of twice the width against weights packed twice per 16-channel group, and the 77-key
                             * cross-attention runs at split precision inside the query projection, LayerNorms folded through an HL16 shadow of the stream.
                             * ~12 % faster than _F32_SPLIT on such weights; falls back to it
                             * on others (sdxl_unet_mix_classes: 0)                                                                                              */
};
/* sdxl_debug_set knobs ("mix_classes", "hl_demote", "hl_tile96", "igemm_*", "attn_*") are PROCESS-WIDE atomics read when a model is built / planned: A/B and
 * measurement tools only, never set them around handles other threads are creating */

/* UNetConfig (src/model/unet/mod.rs:59-69) + DiffuserConfig.is_refiner (src/model/stablediffusion/mod.rs:269-278) */
typedef struct {
  int32_t adm_in_channels, in_channels, out_channels, model_channels;
  int32_t n_levels;
  int32_t channel_mults[8];
  int32_t n_head_channels;
  int32_t transformer_depths[8];
  int32_t context_dim;
  int32_t is_refiner;
} sdxl_unet_config;

/* AutoencoderConfig (src/model/autoencoder/mod.rs:24-44; the reference hard-codes the SDXL values) + LatentDecoderConfig */
typedef struct {
  int32_t n_blocks;
  int32_t enc_in[8], enc_out[8];   /* EncoderConfig channels */
  int32_t dec_in[8], dec_out[8];   /* DecoderConfig channels */
  int32_t n_group, enc_out_channels;
  double scale_factor;             /* LatentDecoderConfig.scale_factor (stablediffusion/mod.rs:176-179), 0.13025 */
} sdxl_vae_config;

/* CLIPConfig (src/model/clip/mod.rs:19-28); SDXL: CLIP ViT-L/14 text {49408,768,768,12,77,12,1} and OpenCLIP ViT-bigG/14
 * text {49408,1280,1280,20,77,32,0} */
typedef struct {
  int32_t n_vocab, n_state, embed_dim, n_head, n_ctx, n_layer;
  int32_t quick_gelu;
} sdxl_clip_config;

/* Conditioning<B> (src/model/stablediffusion/mod.rs:544-555): device fp32 tensors, same ranks as the reference */
typedef struct {
  const float* unconditional_context_full;            /* [77, ctx_full]        */
  const float* unconditional_context_open_clip;       /* [77, 1280]            */
  const float* context_full;                          /* [n, 77, ctx_full]     */
  const float* context_open_clip;                     /* [n, 77, 1280]         */
  const float* unconditional_channel_context;         /* [adm]                 */
  const float* unconditional_channel_context_refiner; /* [adm_refiner]         */
  const float* channel_context;                       /* [n, adm]              */
  const float* channel_context_refiner;               /* [n, adm_refiner]      */
  int32_t n;                                          /* batch of prompts      */
  int32_t n_ctx;                                      /* tokens: 77 per chunk  */
  int32_t height, width;                              /* resolution: [usize;2] */
} sdxl_conditioning;

/* parameter kinds reported by sdxl_*_param_spec */
enum { SDXL_PARAM_LINEAR_W = 0, SDXL_PARAM_CONV_W = 1, SDXL_PARAM_BIAS = 2, SDXL_PARAM_GAMMA = 3, SDXL_PARAM_BETA = 4,
       SDXL_PARAM_EPS = 5 /* [1]: the norm's eps, read per module by the reference (groupnorm/load.rs:19, layernorm/load.rs:17) */ };

const char* sdxl_last_error(void);
/* library / build identification (target arch string, e.g. "gfx950") */
const char* sdxl_build_info(void);

/* one context per GPU (the reference hard-codes LibTorchDevice::Cuda(0), src/bin/sample/main.rs:131) */
int sdxl_ctx_create(int device_id, sdxl_ctx** out);
void sdxl_ctx_destroy(sdxl_ctx* ctx);
int sdxl_ctx_synchronize(sdxl_ctx* ctx);

/* default configs (implied .cfg values) */
void sdxl_unet_config_base(sdxl_unet_config* cfg);
void sdxl_unet_config_refiner(sdxl_unet_config* cfg);
void sdxl_vae_config_default(sdxl_vae_config* cfg);

/* ---- parameter enumeration: replaces the .npy tree walk of src/model/unet/load.rs:286-401, autoencoder/load.rs:186-201 */
int sdxl_unet_param_count(const sdxl_unet_config* cfg);
int sdxl_unet_param_spec(const sdxl_unet_config* cfg, int index, const char** name, int* ndim, int64_t shape[4],
                         int* kind, float* synth_scale, float* synth_mean);
int sdxl_vae_param_count(const sdxl_vae_config* cfg, int encoder);
int sdxl_vae_param_spec(const sdxl_vae_config* cfg, int encoder, int index, const char** name, int* ndim,
                        int64_t shape[4], int* kind, float* synth_scale, float* synth_mean);

/* ---- UNet: replaces DiffuserConfig::init + load_record (stablediffusion/mod.rs:281-305, bin/sample/main.rs:35-43) */
int sdxl_unet_create(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat, sdxl_unet** out);
/* the same from a flat IEEE-f16 buffer (host or device), same order and layouts: burn's HalfPrecisionSettings records hold
 * the weights as f16 (src/bin/sample/main.rs:37, src/bin/convert/main.rs:65-70), so a Rust host hands them over without the
 * 2x fp32 expansion (5.1 GB instead of 10.3 GB for the base UNet).  Likewise sdxl_{diffuser,vae,clip}_create_f16. */
int sdxl_unet_create_f16(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const uint16_t* weights_flat_f16, sdxl_unet** out);
/* seeded synthetic weights generated on the device (no checkpoint needed); bit-identical to oracle/config.py.
 * seed | SDXL_SEED_F16_WEIGHTS: every parameter is rounded to IEEE f16 first (and widened again) -- what a burn
 * HalfPrecisionSettings record holds (src/bin/sample/main.rs:37); the per-norm eps (a module constant) is not. */
#define SDXL_SEED_F16_WEIGHTS (1ull << 63)
int sdxl_unet_create_synthetic(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, uint64_t seed, sdxl_unet** out);
void sdxl_unet_destroy(sdxl_unet* u);
/* UNet::forward(x, timesteps, context, label) -> Tensor<B,4>   (src/model/unet/mod.rs:450-492)
 * x [B,in,H,W], timesteps int32 [B] (device), context [B,n_ctx,ctx_dim], label [B,adm], out [B,out,H,W] */
int sdxl_unet_forward(sdxl_unet* u, void* stream, const float* x, const int32_t* timesteps, const float* context,
                      const float* label, int B, int H, int W, int n_ctx, float* out);
int sdxl_unet_set_graph(sdxl_unet* u, int enabled);   /* hipGraph replay of the forward (default on) */
/* per-handle option (default off): a batch-2 forward -- the CFG pair of forward_diffuser, stablediffusion/mod.rs:523-537 --
 * runs as two concurrent batch-1 chains on two streams inside the captured graph, the second released after
 * `release_offset` GEMM launches of the first.  Bit-identical results; measured -2.6 % step time. */
int sdxl_unet_set_split_cfg(sdxl_unet* u, int enabled, int release_offset);
/* per-handle option (default on, f16 engines): the transformer blocks' cross-attention (unet/mod.rs:731-795) runs inside the
 * epilogue of the query projection instead of as its own kernel.  Off = projection + attention kernel.  Up to 96 context keys
 * (one 77-token prompt chunk) every epilogue form takes it; 97 .. 384 keys (two to four chunks) the f16 engine's weights-in-registers
 * form walks the context in 96-key blocks with an online softmax (widths that are multiples of 128, whole 64-row blocks per entry;
 * knob "xattn_long"); the split-precision form and every other shape run projection + attention kernel above 96 keys, as do all
 * contexts above 384. */
int sdxl_unet_set_fused_cross_attention(sdxl_unet* u, int enabled);
/* per-handle option (default on, f16 engines): GroupNorm statistics come out of the producing convolution's epilogue where
 * its kernel can leave them (256-row tiles: the 64^2 / 32^2 levels at 1024^2) -- groupnorm/mod.rs:52-82 without the statistics pass.
 * Like the two options above it is part of the plan: changing it re-sizes the arena and rebuilds the captured graph on the next forward. */
int sdxl_unet_set_gn_from_producer(sdxl_unet* u, int enabled);
/* which GEMM classes of a SDXL_DTYPE_F32_SPLIT_MIX* model run on plain f16 operands (bit set: 1 self-attention, 2 GEGLU projection, 4 QKV projection,
 * 8 FF-out, 16 / 32 the self- / cross-attention out-projections, 128 cross-attention query projection, 256 LayerNorms folded through an f16 shadow of
 * the stream, 512 the 77-key cross-attention at split precision inside the query projection's epilogue; 0 for every other dtype).  A SDXL_DTYPE_F32_SPLIT_MIX_F16W model whose parameters are NOT all f16 values (checked on the tensors at
 * create time) falls back to SDXL_DTYPE_F32_SPLIT_MIX's classes (1 | 2 | 1024 = the GEGLU weights as (hi, lo) f16 pairs along K): this is how a caller sees it. */
int sdxl_unet_mix_classes(sdxl_unet* u, int* classes_out);

/* ---- create-time adapters (LoRA): the model is built from base weights + sum of scale * left @ right, merged on the device while the
 * weights are packed.  The result is a static merged model: nothing on the per-step path changes and nothing is paid per step.
 * An entry adds scale * left[rows, rank] @ right[rank, cols] to the MATRIX VIEW of parameter `param_index` (sdxl_unet_param_spec order):
 * rows = shape[0], cols = the product of the remaining dimensions.  In terms of the usual PyTorch adapter tensors
 * (down.weight [r, in...], up.weight [out, r]):
 *   SDXL_PARAM_LINEAR_W [d_in, d_out]:       left = down.weight^T [d_in, r],  right = up.weight^T [r, d_out]
 *   SDXL_PARAM_CONV_W   [Cout, Cin, kh, kw]: left = up.weight [Cout, r],      right = down.weight flattened to [r, Cin * kh * kw]
 * left / right: contiguous fp32, host or device (the rule of weights_flat); they are read during the create call only.  Entries on the same
 * parameter are applied in the order given.  The fused QKV / KV packing, GEGLU interleave and every other packed form are the engine's business:
 * an entry always addresses one canonical parameter.
 * Arithmetic (fixed, so a merged model is reproducible): per element acc = 0; acc = fma(left[r][j], right[j][c], acc) for j = 0 .. rank-1;
 * w = fma(scale, acc, w), all fp32.  scale == 0 leaves the tensor untouched.
 * SDXL_LORA_ROUND_F16: every ADAPTED tensor is rounded to IEEE f16 and widened again after its last entry -- what a half-precision record saved
 * after merging would hold.  Merged tensors are in general not f16 values, so without the flag SDXL_DTYPE_F32_SPLIT_MIX_F16W, _GEGLU2 and
 * SDXL_DTYPE_F32_SPLIT_F16W fall back exactly as for any checkpoint that is not f16-valued (sdxl_unet_mix_classes tells); with it they keep their classes
 * (given an f16-valued base). */
typedef struct { int32_t param_index, rank; const float* left; const float* right; float scale; } sdxl_lora_entry;
enum { SDXL_LORA_ROUND_F16 = 1 };
/* host logic only, no device: every entry names a LINEAR_W / CONV_W parameter of cfg, rank >= 1, non-NULL arrays, finite scale.
 * SDXL_ERR_INVALID with the first complaint in sdxl_last_error() otherwise.  n_entries == 0 is valid. */
int sdxl_lora_check(const sdxl_unet_config* cfg, const sdxl_lora_entry* entries, int n_entries);
/* the single op the models run (parity tests): w_dev [rows, cols] fp32 on the device, in place; left [rows, rank], right [rank, cols] host or device;
 * flags: SDXL_LORA_ROUND_F16 rounds w_dev afterwards */
int sdxl_lora_merge(sdxl_ctx* ctx, void* stream, float* w_dev, int rows, int cols, const float* left, const float* right,
                    int rank, float scale, int flags);
/* sdxl_unet_create / _create_f16 / _create_synthetic with adapters.  Exactly one base: weights_flat, weights_flat_f16, or (both NULL) the synthetic
 * seed.  Both bases non-NULL, an entry sdxl_lora_check refuses or unknown flag bits: SDXL_ERR_INVALID, nothing is created, *out is untouched.
 * n_entries == 0 gives the same bits as the plain create call. */
int sdxl_unet_create_lora(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat, const uint16_t* weights_flat_f16,
                          uint64_t synthetic_seed, const sdxl_lora_entry* entries, int n_entries, int flags, sdxl_unet** out);

/* ---- Backend::qkv_attention (src/backend.rs:4-19; generic body :88-128, LibTorch override :32-79)
 * q [B,Nq,n_head*d], k,v [B,Nk,n_head*d], mask additive [Nq,Nk] or NULL, out [B,Nq,n_head*d]; fp32 device tensors.
 * dtype SDXL_DTYPE_F32_SPLIT: d = 64 and mask == NULL only (the UNet's attention), anything else is refused with an error. */
int sdxl_qkv_attention(sdxl_ctx* ctx, void* stream, const float* q, const float* k, const float* v, const float* mask,
                       int B, int Nq, int Nk, int n_state, int n_head, int dtype, float* out);
/* Backend::attn_decoder_mask (src/backend.rs:130-136): writes the [n,n] causal mask (0 / -inf) */
int sdxl_attn_decoder_mask(sdxl_ctx* ctx, void* stream, int seq_length, float* out);

/* ---- Diffuser (src/model/stablediffusion/mod.rs:308-542); alphas_cumprod = alpha_cumulative_products param (:311) */
int sdxl_diffuser_create(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat,
                         const float* alphas_cumprod_host, int n_train_steps, sdxl_diffuser** out);
int sdxl_diffuser_create_f16(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const uint16_t* weights_flat_f16,
                             const float* alphas_cumprod_host, int n_train_steps, sdxl_diffuser** out);
int sdxl_diffuser_create_synthetic(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, uint64_t seed,
                                   const float* alphas_cumprod_host, int n_train_steps, sdxl_diffuser** out);
/* the Diffuser with create-time adapters on its UNet: arguments and errors as sdxl_unet_create_lora */
int sdxl_diffuser_create_lora(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* weights_flat, const uint16_t* weights_flat_f16,
                              uint64_t synthetic_seed, const sdxl_lora_entry* entries, int n_entries, int flags,
                              const float* alphas_cumprod_host, int n_train_steps, sdxl_diffuser** out);
void sdxl_diffuser_destroy(sdxl_diffuser* d);
sdxl_unet* sdxl_diffuser_unet(sdxl_diffuser* d);   /* Diffuser.diffusion (:312), borrowed */
/* Diffuser::sample_latent(conditioning, cfg, n_steps) (:317-332).  noise0 [n,4,h/8,w/8] plays gen_noise() (:378-388). */
int sdxl_sample_latent(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond, double unconditional_guidance_scale,
                       int n_steps, const float* noise0, float* out_latent);
/* Diffuser::sample_latent_with_inpainting (:334-353, loop :434-483).  mask: uint8 [n,4,h/8,w/8], 1 = keep generated.
 * step_noise [iterations, n,4,h/8,w/8]: the per-step gen_noise() of :463 (iterations = sdxl_step_count). */
int sdxl_sample_latent_with_inpainting(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond,
                                       double unconditional_guidance_scale, int n_steps, const float* reference,
                                       const uint8_t* mask, const float* noise0, const float* step_noise,
                                       float* out_latent);
/* Diffuser::refine_latent(latent, conditioning, cfg, step_start, n_steps) (:355-376) */
int sdxl_refine_latent(sdxl_diffuser* d, void* stream, const float* latent, const sdxl_conditioning* cond,
                       double unconditional_guidance_scale, int step_start, int n_steps, const float* noise,
                       float* out_latent);
/* ---- seeded noise: the same three calls with gen_noise() played by a counter-based generator on the device.
 * Philox4x32-10, key = (low, high) 32 bits of the batch entry's seed, counter = (hw, draw, 0, 0) with hw the row-major pixel
 * index of the h/8 x w/8 latent: one counter yields the four channel values of that pixel (two Box-Muller pairs).  The same
 * seed gives the same bits for the same entry, resolution and library build, whatever the batch size and the entry's place
 * in the batch.  `draw` numbers the tensors of one trajectory: */
#define SDXL_DRAW_INITIAL 0u                     /* noise0 of sampling, the re-noise of refine_latent */
#define SDXL_DRAW_BLEND(i) (1u + 2u * (i))       /* inpainting blend in front of iteration i (:463) */
#define SDXL_DRAW_SIGMA(i) (2u + 2u * (i))       /* the gen_noise() * sigma term of iteration i (:427) */
/* gen_noise (:378-388) with a seed: out [n,4,h,w] fp32 (device); seeds: host array [n], one per batch entry */
int sdxl_gen_noise(sdxl_ctx* ctx, void* stream, const uint64_t* seeds, uint32_t draw, int n, int h, int w, float* out);
/* eta in [0, 1] scales sigma of :423-427 (the reference pins it to 0): sigma_t = eta sqrt((1-ap)/(1-a)) sqrt(1-a/ap) and
 * x = x0 sqrt(ap) + e sqrt(1-ap-sigma^2) + z sigma.  The blend and sigma noise are drawn inside the per-step kernel and never
 * stored.  seeds == NULL or eta outside [0, 1] (NaN included): SDXL_ERR_INVALID. */
int sdxl_sample_latent_seeded(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond, double unconditional_guidance_scale,
                              int n_steps, const uint64_t* seeds, double eta, float* out_latent);
int sdxl_sample_latent_with_inpainting_seeded(sdxl_diffuser* d, void* stream, const sdxl_conditioning* cond,
                                              double unconditional_guidance_scale, int n_steps, const float* reference,
                                              const uint8_t* mask, const uint64_t* seeds, double eta, float* out_latent);
int sdxl_refine_latent_seeded(sdxl_diffuser* d, void* stream, const float* latent, const sdxl_conditioning* cond,
                              double unconditional_guidance_scale, int step_start, int n_steps, const uint64_t* seeds,
                              double eta, float* out_latent);
/* number of UNet evaluations of `(0..n_train-step_start).rev().step_by(n_train/n_steps)` (:400-406): 30 -> 31 */
int sdxl_step_count(int n_steps, int step_start, int n_train_steps);
/* ---- solver: the update behind every UNet evaluation, a per-handle option all six trajectory calls above honour.
 * SDXL_SOLVER_DDIM (default) is the reference's loop.  SDXL_SOLVER_DPMPP_2M is DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2;
 * eta > 0: its SDE form, k-diffusion's dpmpp_2m_sde with the midpoint rule, in alpha / sigma terms) on the SAME schedule: one
 * UNet evaluation per iteration, second-order accurate, so it needs about half of DDIM's iterations.  With a = alphas[t_i],
 * ap = alphas[t_i - step] (1 on the last iteration), alpha = sqrt(a), sigma = sqrt(1-a), lambda = ln(alpha / sigma), primes
 * for ap, h = lambda' - lambda, r = h_prev / h, e the CFG-combined noise prediction, x0 = (x - sigma e) / alpha, x0p the x0 of
 * the previous iteration and z a unit normal:
 *     x' = c_x x + c_0 x0 + c_1 x0p + c_z z
 *     A   = -expm1(-(1 + eta) h)      c_x = (sigma' / sigma) exp(-eta h)      c_z = sigma' sqrt(-expm1(-2 eta h))
 *     second order:  c_0 = alpha' A (1 + 1/(2r)),  c_1 = -alpha' A / (2r)
 *     first order:   c_0 = alpha' A,               c_1 = 0
 * First order on iteration 0 of a trajectory (refine_latent's included: no history) and where ap == 1 (h infinite: the row is
 * (0, 1, 0, 0), the iteration returns x0); second order everywhere else.  At eta = 0 a first-order row equals DDIM's.  The
 * draw numbers do not change: SDXL_DRAW_SIGMA(i) is the z of iteration i for both solvers, drawn where c_z != 0; with explicit
 * noise eta is 0.  Inpainting keeps its blend in front of every iteration; x0p is the x0 computed from the blended state. */
enum { SDXL_SOLVER_DDIM = 0, SDXL_SOLVER_DPMPP_2M = 1, SDXL_SOLVER_LCM = 3, SDXL_SOLVER_TCD = 4,
       SDXL_SOLVER_DPMPP_3M = 5 };   /* 2 is not a solver: it stays refused.  DPMPP_3M: the noise-level section below */
/* unknown value: SDXL_ERR_INVALID ("solver" in sdxl_last_error), the handle keeps its solver */
int sdxl_diffuser_set_solver(sdxl_diffuser* d, int solver);
int sdxl_diffuser_get_solver(sdxl_diffuser* d, int* solver_out);
/* host logic only, no device needed: (c_x, c_0, c_1, c_z) as f64 per iteration, out[4*i ..], for i < sdxl_step_count(n_steps,
 * step_start, n_train_steps) <= capacity_steps -- the numbers the sampler rounds to fp32 for its DPM-Solver++(2M) table.  For
 * SDXL_SOLVER_DDIM the same four numbers of the DDIM update: (sqrt(1-ap-sigma_t^2) / sigma, sqrt(ap) - sqrt(1-ap-sigma_t^2)
 * alpha / sigma, 0, sigma_t).  eta outside [0, 1] (NaN included), n_steps outside 1..n_train_steps, step_start outside
 * 0..n_train_steps-1, capacity_steps too small, an unknown solver, alphas outside (0, 1): SDXL_ERR_INVALID, out untouched. */
int sdxl_solver_coefficients(const float* alphas_cumprod_host, int n_train_steps, int n_steps, int step_start, int solver,
                             double eta, double* out, int capacity_steps);
/* ---- prediction type: what the UNet's output means, a per-handle option (refiner handles too) all six trajectory calls above honour, with
 * both solvers, explicit and seeded noise, eta, inpainting, refine_latent and every guidance option.  SDXL_PREDICTION_EPSILON (default) is
 * the reference's reading, the noise e, and a handle that never calls the setter runs exactly what it ran before the option existed.
 * SDXL_PREDICTION_V reads v = alpha e - sigma x0 (Salimans & Ho 2022), what checkpoints trained on a zero-terminal-SNR schedule predict
 * (Lin et al. 2023).  The two branches of an iteration are combined by the guidance lines below as they stand, on v (v = vc; v =
 * fma(vc - vu, s_b, vu), then v f_b: CFG rescale sees the network's raw output rows whatever they mean, under v the moments of vc and vcfg).  Then
 *     x0 = fma(x, alpha, -(v sigma))        no division: finite at alpha == 0, where x0 = -v
 *     e  = fma(v, alpha, x sigma)           SDXL_SOLVER_DDIM only; SDXL_SOLVER_DPMPP_2M never forms e
 * and everything behind x0 and e -- the DDIM / 2M update, the sigma noise, the inpainting blend -- is unchanged: the rows (c_x, c_0, c_1,
 * c_z) do not depend on the prediction type.
 * Zero terminal SNR: with a = alphas_cumprod at an iteration's own timestep, a == 0 is admitted under SDXL_PREDICTION_V (ap == 0 and
 * a >= 1 stay refused), and such a table can be handed to sdxl_diffuser_create* as it is.  There alpha = 0, sigma = 1, lambda = -inf and
 * h = +inf, and the rows are the limits: DDIM's expressions are finite as they stand (sigma_t = eta sqrt(1 - ap)); the 2M row is first
 * order, (sigma', alpha', 0, 0) at eta == 0 and (0, alpha', 0, sigma') at eta > 0, and the iteration behind it (r = h_prev / h = inf) is first
 * order too, like iteration 0.  Under SDXL_PREDICTION_EPSILON a trajectory, replay or coefficient call whose schedule touches a timestep
 * with a == 0 returns SDXL_ERR_INVALID before anything is launched (x0 would divide by alpha == 0); the message names v-prediction. */
enum { SDXL_PREDICTION_EPSILON = 0, SDXL_PREDICTION_V = 1 };   /* (x0 / "sample" and EDM parameterisations: not offered, values 2.. are free) */
/* unknown value: SDXL_ERR_INVALID ("prediction" in sdxl_last_error), the handle keeps its own */
int sdxl_diffuser_set_prediction(sdxl_diffuser* d, int prediction);
int sdxl_diffuser_get_prediction(sdxl_diffuser* d, int* prediction_out);
/* host logic only: Lin et al. 2023, Algorithm 1 on s = sqrt(alphas_cumprod) in f64:
 * s <- (s - s[T-1]) * s[0] / (s[0] - s[T-1]);  out = (float)(s * s).  out[T-1] is exactly 0, out[0] == in[0] as a float.
 * n < 2, NULL, an input outside (0, 1) or not strictly decreasing: SDXL_ERR_INVALID, out untouched.  in == out allowed. */
int sdxl_rescale_zero_terminal_snr(const float* alphas_cumprod_in, int n_train_steps, float* alphas_cumprod_out);
/* sdxl_solver_coefficients under a prediction type: the same rows, and with SDXL_PREDICTION_V the a == 0 rows above.  An unknown prediction,
 * or SDXL_PREDICTION_EPSILON with a == 0 at an iteration's timestep: SDXL_ERR_INVALID, out untouched.  sdxl_solver_coefficients is this
 * entry with SDXL_PREDICTION_EPSILON. */
int sdxl_solver_coefficients_pred(const float* alphas_cumprod_host, int n_train_steps, int n_steps, int step_start, int solver,
                                  int prediction, double eta, double* out, int capacity_steps);
/* ---- few-step sampling: timestep lists and the consistency solvers (distilled checkpoints: LCM / TCD / Hyper-SD LoRAs through
 * sdxl_diffuser_create_lora, Turbo, Lightning; usually with SDXL_GUIDANCE_OFF or a guidance scale near 1).
 *
 * Timestep list.  A trajectory is one UNet evaluation per entry of a strictly decreasing list t_0 > t_1 > ... > t_{n-1} of training
 * timesteps, and the list is the only source of an iteration's numbers: a = alphas[t_i], ap = alphas[t_{i+1}], ap = 1 behind the last
 * entry; the guidance interval (t_lo..t_hi), the trace, the step timing and the t fed to the UNet read it too.  Without a list the handle
 * runs the reference's rule, sdxl_step_count's list, for which alphas[t_{i+1}] is the alphas[t_i - step] it always read: a handle that never
 * calls the setter runs exactly what it ran before.  DDIM (with eta) and 2M (ODE and SDE; r = h_prev / h copes with uneven spacing) run on
 * a list through the formulas above.
 * sdxl_diffuser_set_timesteps sets a per-handle list for all six trajectory calls; n == 0 or NULL goes back to the reference's rule.
 * SDXL_ERR_INVALID ("timesteps" in sdxl_last_error), the handle keeping what it had: n outside 1..n_train_steps, a value outside
 * 0..n_train_steps-1, values not strictly decreasing.  With a list set, a trajectory call returns SDXL_ERR_INVALID before anything is
 * launched where its n_steps differs from the list's length (it is not ignored); sampling and inpainting have step_start = 0;
 * sdxl_refine_latent* keeps step_start's meaning for the re-noise level alphas[n_train_steps - step_start] and requires
 * t_0 == n_train_steps - step_start - 1, the reference's own relation between the two.
 * sdxl_diffuser_get_timesteps returns the count written to out, 0 for the reference's rule; capacity too small: SDXL_ERR_INVALID. */
int sdxl_diffuser_set_timesteps(sdxl_diffuser* d, const int32_t* timesteps, int n);
int sdxl_diffuser_get_timesteps(sdxl_diffuser* d, int32_t* out, int capacity);
/* host logic only: the published spacings as lists.  Returns the count written, or SDXL_ERR_INVALID with out untouched (NULL, n_steps
 * outside 1..n_train_steps, capacity smaller than the count, an unknown kind, and what each kind refuses).  Integer arithmetic (C division)
 * except where stated; i = 0 .. count-1:
 *   SDXL_SCHEDULE_REFERENCE  t_i = n_train - 1 - i (n_train / n_steps) while >= 0; count = sdxl_step_count(n_steps, 0, n_train): 30 -> 31
 *   SDXL_SCHEDULE_TRAILING   t_i = rint(n_train - i q) - 1 in f64, q = n_train / n_steps in f64, ties to even (diffusers "trailing", numpy's
 *                            round); count n_steps; 4 -> 999, 749, 499, 249 (Lightning, Turbo)
 *   SDXL_SCHEDULE_LEADING    t_i = (n_steps - 1 - i) (n_train / n_steps) + param, param = diffusers' steps_offset (1 for SDXL); refused where
 *                            param < 0 or t_0 >= n_train; count n_steps; 4, offset 1 -> 751, 501, 251, 1
 *   SDXL_SCHEDULE_LCM        O = param origin steps (50 for the published LCM / TCD / Hyper-SD checkpoints), k = n_train / O,
 *                            r_j = (O - j) k - 1, t_i = r_floor(i O / n_steps); refused where O < 1, O > n_train or n_steps > O; count n_steps;
 *                            O = 50: 4 -> 999, 759, 499, 259;  8 -> 999, 879, 759, 639, 499, 379, 259, 139
 * A count of 1 and SDXL_ERR_INVALID are the same number (here and in sdxl_diffuser_get_timesteps): a refusal leaves out untouched and no list
 * holds a negative value, so a caller that may get either pre-fills out[0] with -1. */
enum { SDXL_SCHEDULE_REFERENCE = 0, SDXL_SCHEDULE_TRAILING = 1, SDXL_SCHEDULE_LEADING = 2, SDXL_SCHEDULE_LCM = 3 };
int sdxl_timestep_schedule(int kind, int n_steps, int n_train_steps, int param, int32_t* out, int capacity);
/* Consistency solvers.  SDXL_SOLVER_LCM (Luo et al. 2023, multistep consistency sampling) and SDXL_SOLVER_TCD (Zheng et al. 2024,
 * gamma-sampling; what Hyper-SD ships with) jump to a data prediction and re-noise it with fresh noise every iteration.  Both are
 * first-order rows (c_x, c_0, 0, c_z) of x' = c_x x + c_0 x0 + c_z z above, with or without a list (without: on the reference's rule);
 * x0 comes from the epsilon or v lines, z is the SDXL_DRAW_SIGMA(i) tensor, alpha = sqrt(a), sigma = sqrt(1-a), primes for ap.  In the
 * per-step kernel:  acc = x0 c_0 (one rounding);  x = fma(x, c_x, acc);  x = fma(z, c_z, x) where c_z != 0.  No history is kept.
 *   SDXL_SOLVER_LCM  diffusers' LCMScheduler.step with sigma_data = 0.5, timestep_scaling = 10:  s = 10 t,  c_skip = 0.25 / (s^2 + 0.25),
 *                    c_out = s / sqrt(s^2 + 0.25);  row (alpha' c_skip, alpha' c_out, 0, sigma');  behind the last entry ap = 1: (c_skip, c_out,
 *                    0, 0).  eta is not a parameter: the seeded calls, the replay and the coefficient entries return SDXL_ERR_INVALID for
 *                    eta != 0 under this solver.
 *   SDXL_SOLVER_TCD  diffusers' TCDScheduler.step with the seeded calls' eta in [0, 1] read as gamma (as diffusers passes it): with t' the
 *                    next list entry, s = floor((1.0 - gamma) t') in f64, a_s = alphas[s], alpha_s, sigma_s, r = sqrt(ap / a_s):
 *                    row (r sigma_s / sigma,  r (alpha_s - sigma_s alpha / sigma),  0,  sqrt(1 - ap / a_s)).  At gamma = 0, s = t': DDIM's row at
 *                    eta 0, c_z = 0.  Behind the last entry the row is (0, 1, 0, 0), the engine's convention as 2M has it: the trajectory
 *                    returns x0.  (diffusers returns sqrt(a_0) x0 + sqrt(1 - a_0) e there, a latent still at the noise level of timestep 0.)
 * Under SDXL_PREDICTION_V a == 0 at an iteration's own timestep is admitted as above, both rows being finite there as written; under
 * SDXL_PREDICTION_EPSILON it is refused with the message above.  The inpainting blend in front of the next iteration and the draw numbers
 * do not change.  No seeds, no noise: an explicit-noise trajectory call, or a replay without seeds, whose table (at eta = 0) has any
 * c_z != 0 returns SDXL_ERR_INVALID before anything is launched (the message says the solver needs the seeded calls).  Still running on
 * explicit noise: a one-entry LCM list, TCD (gamma = 0 there), and explicit-noise inpainting with every c_z == 0, which keeps its blend. */
/* sdxl_solver_coefficients_pred on a list: n rows for the n entries of timesteps.  SDXL_ERR_INVALID, out untouched: what that entry refuses,
 * a list sdxl_diffuser_set_timesteps refuses, capacity_steps < n, eta != 0 under SDXL_SOLVER_LCM.  The two entries above are this one on the
 * reference's list. */
int sdxl_solver_coefficients_ts(const float* alphas_cumprod_host, int n_train_steps, const int32_t* timesteps, int n, int solver,
                                int prediction, double eta, double* out, int capacity_steps);
/* ---- noise-level schedules: sigma lists, partial trajectories, DPM++ 3M SDE.
 *
 * A trajectory is a list of noise levels with an end level: iteration i runs at alphas_cumprod a_i and lands on ap = a_{i+1}, behind the last
 * entry on the end level (1 = the data itself: the complete trajectory).  A timestep list is the special case a_i = alphas[t_i].
 *
 * Sigma list.  k-diffusion's sigma = sqrt((1 - a) / a), strictly decreasing, finite and > 0; a_i = 1 / (1 + sigma_i^2) in f64 -- a level
 * between two training timesteps.  The timestep of such a level -- what the UNet is fed as a float, what the guidance interval compares
 * (t_lo <= t <= t_hi on the f64 value) and what LCM scales (s = 10 t) -- is k-diffusion's sigma_to_t in f64: with
 * L_j = 0.5 ln((1 - alphas[j]) / alphas[j]), low the largest j <= n_train_steps - 2 with L_j <= ln sigma (0 if there is none), high = low + 1,
 *     w = clamp((L_low - ln sigma) / (L_low - L_high), 0, 1),    t = (1 - w) low + w high.
 * SDXL_SIGMAS_ROUND_T rounds that t to the nearest integer, ties to even (diffusers' use_karras_sigmas convention); a stays the sigma's own.
 * DDIM (Euler-ancestral is DDIM at eta = 1 on the same list), 2M, 3M and LCM run on a sigma list.  TCD reads alphas at floor((1 - gamma) t'),
 * a training timestep: on a sigma list it is refused (SDXL_ERR_INVALID, "sigmas" in sdxl_last_error).
 * The start latent of sampling and inpainting stays the unit-normal tensor it is on a timestep list (noise0, or the SDXL_DRAW_INITIAL draw):
 * it is NOT scaled by sqrt(1 - a_0) or by sigma_0.  A list that starts at the table's sigma_max (14.6 for SDXL, sqrt(1 - a) = 0.998) is the
 * usual case; k-diffusion's x = noise * sigma_max is this tensor in its variance-exploding variables.
 * sdxl_diffuser_set_sigmas: the list of every following trajectory call of the handle, whose n_steps must equal n and whose step_start is 0.
 * sigma_end in [0, sigmas[n-1]) is the level behind the last entry, 0 the complete trajectory.  While a sigma list is set it is the one list
 * in force (sdxl_diffuser_get_timesteps reports none); n == 0 or NULL drops it and the handle is back on the timestep list or rule it had
 * before; sdxl_diffuser_set_timesteps* drops it too.  SDXL_ERR_INVALID ("sigmas" in sdxl_last_error), the handle keeping what it had: n
 * outside 1..n_train_steps, a value that is not finite and > 0, values not strictly decreasing, sigma_end outside its range, unknown flags.
 * sdxl_refine_latent* on a handle with a sigma list is refused: its re-noise level is tied to step_start; the message names sdxl_continue_latent.
 * sdxl_diffuser_get_sigmas returns the count written to out (0: no sigma list; sigma_end_out / flags_out, optional, are then left alone). */
enum { SDXL_SIGMAS_ROUND_T = 1 };
int sdxl_diffuser_set_sigmas(sdxl_diffuser* d, const double* sigmas, int n, double sigma_end, int flags);
int sdxl_diffuser_get_sigmas(sdxl_diffuser* d, double* out, int capacity, double* sigma_end_out, int* flags_out);
/* sdxl_diffuser_set_timesteps with an end level: the last iteration lands on ap = alphas[t_end], -1 <= t_end < timesteps[n-1]; -1 gives ap = 1,
 * and sdxl_diffuser_set_timesteps is this entry with -1.  A t_end outside its range: SDXL_ERR_INVALID ("timesteps"), the handle keeps what it
 * had.  sdxl_diffuser_get_timesteps_end: the handle's t_end, -1 without a list. */
int sdxl_diffuser_set_timesteps_end(sdxl_diffuser* d, const int32_t* timesteps, int n, int t_end);
int sdxl_diffuser_get_timesteps_end(sdxl_diffuser* d, int* t_end_out);
/* host logic only: the published sigma spacings, f64, i = 0 .. count-1.  Returns the count written (the terminal 0 is not part of a list), or
 * SDXL_ERR_INVALID with out untouched.  sigma_min / sigma_max <= 0 take the table's own ends sqrt((1 - a) / a) at timestep 0 and n_train_steps - 1
 * (0.02917 and 14.6146 on SDXL's table).
 *   SDXL_SIGMAS_KARRAS        (smax^(1/rho) + i / (n-1) (smin^(1/rho) - smax^(1/rho)))^rho  (Karras et al. 2022, eq. 5; rho = 7); count n_steps
 *   SDXL_SIGMAS_EXPONENTIAL   exp(ln smax + i / (n-1) (ln smin - ln smax)); count n_steps
 *   SDXL_SIGMAS_OF_TIMESTEPS  the sigma of every entry of SDXL_SCHEDULE_REFERENCE's list; count sdxl_step_count(n_steps, 0, n_train_steps);
 *                             sigma_min, sigma_max and rho are not read
 * n_steps == 1 gives smax.  Refused: NULL, a table of fewer than two entries or with a value outside [0, 1), n_steps outside 1..n_train_steps,
 * not 0 < smin < smax, rho not finite and > 0, an unknown kind, a sigma that is not finite (a == 0 in the table), capacity < count. */
enum { SDXL_SIGMAS_KARRAS = 0, SDXL_SIGMAS_EXPONENTIAL = 1, SDXL_SIGMAS_OF_TIMESTEPS = 2 };
int sdxl_sigma_schedule(int kind, int n_steps, const float* alphas_cumprod_host, int n_train_steps, double sigma_min, double sigma_max,
                        double rho, double* out, int capacity);
/* host logic only: the mapping above as an entry of its own; flags: 0 or SDXL_SIGMAS_ROUND_T.  A sigma that is not finite and > 0, unknown
 * flags, NULL, a table as above: SDXL_ERR_INVALID, t_out untouched. */
int sdxl_sigma_to_timestep(const float* alphas_cumprod_host, int n_train_steps, double sigma, int flags, double* t_out);
/* Continuing a trajectory: the SDXL base -> refiner handoff ("ensemble of expert denoisers") and any other split.  A handle whose list ends on
 * a level (sigma_end > 0, t_end >= 0) returns the latent AT that level; sdxl_continue_latent runs the handle's list -- sigma or timestep; a
 * handle without one is refused, and n_steps must equal its length -- from a given latent [n,4,h/8,w/8]:
 *   renoise == 0   the latent is used as it is: the handoff.  noise is ignored; seeds may be NULL if and only if the table has no c_z != 0
 *                  (eta == 0 under DDIM, 2M and 3M: the explicit-noise rule above).
 *   renoise != 0   the start is sqrt(a_0) latent + sqrt(1 - a_0) z with a_0 the list's first level and z the noise tensor or the
 *                  SDXL_DRAW_INITIAL draw of seeds: exactly one of the two is given.
 * It honours solver, prediction, guidance and eta (in [0, 1], seeds needed where != 0) like the six calls above; there is no inpainting
 * through it.  A multistep solver starts first order here, as on iteration 0 of any trajectory: a 4 + 2 split of a 6-entry list equals the
 * one 6-entry run bit for bit under DDIM at eta 0 and restarts the order under 2M and 3M.  Draw numbers restart too (SDXL_DRAW_SIGMA(i), i
 * counted from the continued list's first entry).  Refusals: SDXL_ERR_INVALID before anything is launched, out untouched. */
int sdxl_continue_latent(sdxl_diffuser* d, void* stream, const float* latent, const sdxl_conditioning* cond,
                         double unconditional_guidance_scale, int n_steps, const float* noise, const uint64_t* seeds, double eta, int renoise,
                         float* out_latent);
/* SDXL_SOLVER_DPMPP_3M: k-diffusion's sample_dpmpp_3m_sde in alpha / sigma terms, the 2M update with one more history term,
 *     x' = c_x x + c_0 x0 + c_1 x0p + c_2 x0pp + c_z z
 * with eta in [0, 1] of the seeded calls (0: the ODE form).  lambda = ln(alpha / sigma), h = lambda' - lambda, h_eta = (1 + eta) h, h1 and h2
 * the previous two h, r0 = h1 / h, r1 = h2 / h:
 *     A = -expm1(-h_eta)     phi2 = expm1(-h_eta) / h_eta + 1     phi3 = phi2 / h_eta - 1/2
 *     c_x = (sigma' / sigma) exp(-eta h)     c_z = sigma' sqrt(-expm1(-2 eta h))
 *     third order (two histories):  P = phi2 (1 + r0 / (r0 + r1)) - phi3 / (r0 + r1),   Q = (phi3 - phi2 r0) / (r0 + r1)
 *         c_0 = alpha' (A + P / r0)     c_1 = alpha' (-P / r0 + Q / r1)     c_2 = -alpha' Q / r1
 *     second order (one history):   c_0 = alpha' (A + phi2 / r0)     c_1 = -alpha' phi2 / r0     c_2 = 0
 *     first order (iteration 0):    c_0 = alpha' A,  c_1 = c_2 = 0
 *     ap == 1:  (0, 1, 0, 0, 0)
 * The order starts at one wherever a trajectory starts (sdxl_continue_latent included) and, under SDXL_PREDICTION_V, behind a row with a == 0
 * (h = +inf), which is 2M's limit row.  In the per-step kernel: acc = c_2 x0pp; acc = fma(x0p, c_1, acc); acc = fma(x0, c_0, acc);
 * x = fma(x, c_x, acc); x = fma(z, c_z, x) where c_z != 0; a history is read only where its coefficient != 0.
 * sdxl_solver_rows: host logic only, (c_x, c_0, c_1, c_2, c_z) as f64 per iteration, out[5*i ..], for any solver on any schedule.  For the
 * solvers above columns 0, 1, 2 and 4 are the numbers of sdxl_solver_coefficients_ts and column 3 is 0.  The four-column entries and
 * sdxl_sampler_step_replay* refuse SDXL_SOLVER_DPMPP_3M; the message names sdxl_solver_rows / sdxl_sampler_step_replay_levels.
 * sdxl_schedule_desc: a schedule as plain data, exactly one of timesteps and sigmas non-NULL, n entries; t_end as in
 * sdxl_diffuser_set_timesteps_end (read with timesteps), sigma_end and flags as in sdxl_diffuser_set_sigmas (read with sigmas).
 * SDXL_ERR_INVALID, out untouched: what the list setters and sdxl_solver_coefficients_ts refuse, TCD on sigmas, capacity_rows < n. */
typedef struct {
  const float* alphas_cumprod_host; int32_t n_train_steps;
  const int32_t* timesteps; const double* sigmas; int32_t n;
  int32_t t_end; double sigma_end; int32_t flags;
} sdxl_schedule_desc;
int sdxl_solver_rows(const sdxl_schedule_desc* schedule, int solver, int prediction, double eta, double* out, int capacity_rows);
/* ---- guidance: how the two UNet branches of an iteration become the noise prediction e, a per-handle option all six trajectory
 * calls above honour, with both solvers, explicit and seeded noise, and inpainting.  The default is the reference's line (:539-540),
 * e = eu + (ec - eu) s with the call's scalar s on every iteration, and a handle with default options runs exactly what it ran before
 * these options existed.  Per batch entry b and iteration i at timestep t_i:
 *   SDXL_GUIDANCE_OFF   the conditional branch alone, e = ec, as a batch-n forward (distilled checkpoints: Turbo, Lightning, LCM).
 *                       The unconditional tensors of sdxl_conditioning may be NULL, the scale argument is ignored, n may reach 8.
 *   inactive iteration  (t_i outside [t_lo, t_hi]; guidance interval, Kynkaanniemi et al. 2024): e = ec exactly.  Both branches
 *                       still run: the batch-2n forward is one captured graph per handle.
 *   active iteration    ecfg = fma(ec - eu, s_b, eu), s_b = scales[b] where n_scales > 0, else the call's scalar;
 *                       rescale = 0: e = ecfg.   rescale = phi > 0 (CFG rescale, Lin et al. 2023, section 3.4):
 *                           e = ecfg f_b,   f_b = fma(phi, r_b, 1 - phi),   r_b = sqrt(M2(ec) / M2(ecfg))
 *                       M2 the centred sum of squares over the 4 HW values of entry b (the ratio of standard deviations, whichever
 *                       of N, N-1 divides them); M2(ecfg) == 0 gives f_b = 1.  f_b has the same bits for an entry alone and batched.
 * Everything behind e -- x0, the DDIM / 2M update, the sigma noise, the inpainting blend -- is unchanged.  Not offered: per-entry
 * negative prompts (the sdxl_conditioning layout holds one unconditional tensor). */
enum { SDXL_GUIDANCE_CFG = 0, SDXL_GUIDANCE_OFF = 1 };
typedef struct {
  int32_t mode;        /* SDXL_GUIDANCE_CFG (default) or SDXL_GUIDANCE_OFF */
  float   rescale;     /* phi in [0, 1]; 0 = off (default) */
  int32_t n_scales;    /* 0 (default: the call's scalar) or the trajectory's cond.n */
  float   scales[8];   /* per-entry guidance scales, replace the call's scalar */
  int32_t t_lo, t_hi;  /* guidance is active on iterations whose timestep t has t_lo <= t <= t_hi; default 0 .. INT32_MAX */
} sdxl_guidance;
void sdxl_guidance_default(sdxl_guidance* g);
/* host logic only, no device.  SDXL_ERR_INVALID with the first complaint in sdxl_last_error() for: an unknown mode; rescale outside
 * [0, 1] (NaN included); n_scales outside 0..8; a non-finite scale; t_lo < 0 or t_lo > t_hi; SDXL_GUIDANCE_OFF together with any
 * other non-default field; is_refiner != 0 with anything but the default or SDXL_GUIDANCE_OFF (the refiner has no unconditional branch). */
int sdxl_guidance_check(const sdxl_guidance* g, int is_refiner);
/* g == NULL: the default.  Options sdxl_guidance_check refuses for this handle: SDXL_ERR_INVALID, the handle keeps its options.
 * A trajectory call with n_scales != 0 && n_scales != cond.n returns SDXL_ERR_INVALID before anything is launched. */
int sdxl_diffuser_set_guidance(sdxl_diffuser* d, const sdxl_guidance* g);
int sdxl_diffuser_get_guidance(sdxl_diffuser* d, sdxl_guidance* out);
/* the single op behind rescale, the two kernels the sampler runs: eps = UNet output rows [2n, HW, 4] fp32 (device; cond entries
 * first), scales: host array [n], 1 <= n <= 8, factors_out: device array [n] that receives f_b.  1 <= HW <= 2^22 (the latent of a
 * 16384 x 16384 image): one wavefront per entry merges the ceil(HW / 256) block partials one after the other, which is what keeps
 * the result reproducible -- 64 merges at 1024 x 1024, and a cost that grows with HW */
int sdxl_cfg_rescale_factors(sdxl_ctx* ctx, void* stream, const float* eps, int n, int HW, const float* scales, float rescale,
                             float* factors_out);
/* the trajectory without the UNet (a test seam: what pins the bits of the per-step kernel): every launch a trajectory call makes between two
 * UNet forwards -- the coefficient table, the initial launch, per iteration the rescale factors and the update -- with the noise predictions
 * given.  iterations = sdxl_step_count(n_steps, step_start, n_train_steps), B = n where single != 0, else 2n.  Host: alphas_cumprod_host
 * [n_train_steps], guidance (NULL: the default), seeds [n] (NULL: explicit noise, eta must be 0).  Device inputs: eps [iterations, B, h*w, 4]
 * fp32 (cond entries first), latent0 [n,4,h,w], and optionally reference [n,4,h,w] + mask uint8 [n,4,h,w] (inpainting; with explicit noise
 * step_noise [iterations, n,4,h,w] too).  Device outputs, all fp32: latents_out [iterations+1, n,4,h,w] (after the initial launch and after
 * every update), hist_out [n,4,h,w] (the x0 history after the last update; SDXL_SOLVER_DPMPP_2M only, else untouched, may be NULL),
 * unet_in_out [B, h*w, 4] (the UNet input after the last launch, kept as f16 in between where input_f16 != 0), timesteps_out [iterations+1].
 * SDXL_ERR_INVALID before anything is launched: a NULL required pointer, n outside 1..8, h*w outside 1..2^22, a solver, eta, schedule or
 * alphas sdxl_solver_coefficients refuses, mask without reference (or the reverse), explicit-noise inpainting without step_noise, eta != 0
 * without seeds, options sdxl_guidance_check refuses (single != 0 takes the default or SDXL_GUIDANCE_OFF only), n_scales != 0 && != n. */
typedef struct {
  const float* alphas_cumprod_host; int32_t n_train_steps, n_steps, step_start;
  int32_t solver; double eta; double unconditional_guidance_scale;
  const sdxl_guidance* guidance; int32_t single;
  int32_t n, h, w; int32_t input_f16;
  const float* eps; const float* latent0; const float* reference; const uint8_t* mask; const float* step_noise; const uint64_t* seeds;
  float* latents_out; float* hist_out; float* unet_in_out; float* timesteps_out;
} sdxl_step_replay_args;
int sdxl_sampler_step_replay(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* args);
/* the same replay with eps read under `prediction` (SDXL_PREDICTION_V: the rows are v); sdxl_sampler_step_replay is this entry with
 * SDXL_PREDICTION_EPSILON.  The struct is shared.  Refuses what sdxl_solver_coefficients_pred refuses. */
int sdxl_sampler_step_replay_pred(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* args, int prediction);
/* the same replay on a list: iterations = n, and the struct's n_steps and step_start are ignored (timesteps == NULL or n == 0: they are
 * read, and this is sdxl_sampler_step_replay_pred).  The struct's layout is shared.  Refuses, before anything is launched, what that entry
 * refuses, a list sdxl_diffuser_set_timesteps refuses, eta != 0 under SDXL_SOLVER_LCM, and seeds == NULL with any c_z != 0 in the table.
 * hist_out stays untouched under SDXL_SOLVER_LCM and SDXL_SOLVER_TCD: they keep no history. */
int sdxl_sampler_step_replay_ts(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* args, int prediction, const int32_t* timesteps,
                                int n);
/* the same replay on any schedule and with any solver: iterations = schedule->n; the struct's alphas_cumprod_host, n_train_steps, n_steps and
 * step_start are ignored (the schedule carries the table).  timesteps_out holds (float)t of every entry, fractional on a sigma list, and 0
 * behind the last.  hist_out / hist2_out [n,4,h,w], both optional: the x0 histories after the last update -- hist_out the last x0 under
 * SDXL_SOLVER_DPMPP_2M and _3M; hist2_out, under _3M and with at least two iterations, the x0p of the last update that read one (the x0 in
 * front of hist_out's unless the last row is the ap == 1 row or restarts the order).  They stay untouched where the solver keeps none.
 * An integer list with t_end = -1 gives the bits of sdxl_sampler_step_replay_ts.  Refuses what sdxl_solver_rows and that entry refuse. */
int sdxl_sampler_step_replay_levels(sdxl_ctx* ctx, void* stream, const sdxl_step_replay_args* args, int prediction,
                                    const sdxl_schedule_desc* schedule, float* hist2_out);
/* per-iteration GPU milliseconds of the last trajectory (enable first); returns the number written */
int sdxl_diffuser_enable_step_timing(sdxl_diffuser* d, int enabled);
int sdxl_diffuser_step_times(sdxl_diffuser* d, float* out_ms, int capacity);
/* parity instrumentation: after DDIM iteration i (< capacity_steps) of every following trajectory the latent [n,4,h/8,w/8]
 * is copied to trace_dev + i * numel (device buffer owned by the caller); NULL / 0 switches it off.  These are the
 * per-step latents `diffuse_latent` rebinds at stablediffusion/mod.rs:424-428.  With inpainting the copy is taken behind the fused
 * DDIM kernel, i.e. it already carries the blend of the NEXT iteration outside the mask (:463-465); the last one carries none. */
int sdxl_diffuser_set_trace(sdxl_diffuser* d, float* trace_dev, int capacity_steps);

/* ---- LatentDecoder / Autoencoder (stablediffusion/mod.rs:193-267, autoencoder/mod.rs:46-70) */
int sdxl_vae_create(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, const float* decoder_weights_flat,
                    const float* encoder_weights_flat, sdxl_vae** out);   /* either side may be NULL */
int sdxl_vae_create_f16(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, const uint16_t* decoder_weights_flat_f16,
                        const uint16_t* encoder_weights_flat_f16, sdxl_vae** out);
int sdxl_vae_create_synthetic(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, uint64_t seed, int with_encoder,
                              sdxl_vae** out);
void sdxl_vae_destroy(sdxl_vae* v);
/* LatentDecoder::decode_latent (:263-266): latent [n,4,h,w] -> image [n,3,8h,8w] */
int sdxl_vae_decode_latent(sdxl_vae* v, void* stream, const float* latent, int n, int h, int w, float* out_image);
/* LatentDecoder::latent_to_image (:200-237): -> RawImages.buffer, uint8 [n,8h,8w,3] (device) */
int sdxl_latent_to_image(sdxl_vae* v, void* stream, const float* latent, int n, int h, int w, uint8_t* out_hwc);
/* LatentDecoder::encode_image (:257-261): image [n,3,H,W] in [-1,1] -> latent [n,4,H/8,W/8] */
int sdxl_vae_encode_image(sdxl_vae* v, void* stream, const float* image, int n, int H, int W, float* out_latent);
/* LatentDecoder::image_to_latent (:239-255): uint8 [n,H,W,3] (device) -> latent */
int sdxl_image_to_latent(sdxl_vae* v, void* stream, const uint8_t* image_hwc, int n, int H, int W, float* out_latent);

/* ---- Embedder (stablediffusion/mod.rs:626-801): the two CLIP text encoders.  Tokenisation stays with the caller (host
 * string code: src/token/{clip,open_clip}.rs) -- token ids cross the boundary, as in the reference's CLIP::forward_* */
void sdxl_clip_config_clip_l(sdxl_clip_config* cfg);
void sdxl_clip_config_open_clip_bigg(sdxl_clip_config* cfg);
/* parameter enumeration, replaces clip/load.rs:  token_embedding.weight [n_vocab,n_state], position_embedding [n_ctx,n_state],
 * blocks.{i}.{attn.{query,key,value,out}, attn_ln, mlp.{fc1,fc2}, mlp_ln}, layer_norm, text_projection [n_state,embed_dim] */
int sdxl_clip_param_count(const sdxl_clip_config* cfg);
int sdxl_clip_param_spec(const sdxl_clip_config* cfg, int index, const char** name, int* ndim, int64_t shape[4], int* kind,
                         float* synth_scale, float* synth_mean);
/* CLIPConfig::init + load (clip/mod.rs:30-59) */
int sdxl_clip_create(sdxl_ctx* ctx, const sdxl_clip_config* cfg, int dtype, const float* weights_flat, sdxl_clip** out);
int sdxl_clip_create_f16(sdxl_ctx* ctx, const sdxl_clip_config* cfg, int dtype, const uint16_t* weights_flat_f16, sdxl_clip** out);
int sdxl_clip_create_synthetic(sdxl_ctx* ctx, const sdxl_clip_config* cfg, int dtype, uint64_t seed, sdxl_clip** out);
void sdxl_clip_destroy(sdxl_clip* c);
/* CLIP::forward_hidden (clip/mod.rs:94-112): tokens int32 [n,seq] (device) -> hidden [n,seq,n_state] after the first
 * hidden_idx blocks, no final LayerNorm */
int sdxl_clip_forward_hidden(sdxl_clip* c, void* stream, const int32_t* tokens, int n, int seq, int hidden_idx, float* out_hidden);
/* CLIP::forward_hidden_pooled (clip/mod.rs:114-151): hidden = input of block hidden_idx [n,seq,n_state];
 * pooled [n,embed_dim] = layer_norm(x_final)[argmax(tokens)] @ text_projection */
int sdxl_clip_forward_hidden_pooled(sdxl_clip* c, void* stream, const int32_t* tokens, int n, int seq, int hidden_idx,
                                    float* out_hidden, float* out_pooled);
/* conditioning_embedding (unet/mod.rs:41-57): pooled [n,E] and int32 values [n,w] (size|crop|ar, device) ->
 * out [n, E + w*dim] = [pooled | timestep_embedding(values, dim)] */
int sdxl_conditioning_embedding(sdxl_ctx* ctx, void* stream, const float* pooled, int n, int E, const int32_t* values, int w,
                                int dim, float* out);
int sdxl_clip_weight_arena(sdxl_clip* c, void** base, size_t* bytes);

/* ---- multi-GPU: the packed weight arena of a model, for a one-time RCCL broadcast from rank 0 (SURVEY 2.3 C-bcast).
 * Replica ranks create the model "empty" (identical arena layout, contents undefined) and receive the bytes. */
int sdxl_unet_weight_arena(sdxl_unet* u, void** base, size_t* bytes);
int sdxl_vae_weight_arena(sdxl_vae* v, void** base, size_t* bytes);
int sdxl_diffuser_create_empty(sdxl_ctx* ctx, const sdxl_unet_config* cfg, int dtype, const float* alphas_cumprod_host,
                               int n_train_steps, sdxl_diffuser** out);
int sdxl_vae_create_empty(sdxl_ctx* ctx, const sdxl_vae_config* cfg, int dtype, int with_encoder, sdxl_vae** out);

/* ---- one-time weight broadcast over RCCL / xGMI (the reference is single-device, sample/main.rs:131).
 * One process per GPU.  Rank 0 calls sdxl_comm_unique_id and ships the 128 bytes to the other ranks by any host channel;
 * every rank then creates its communicator and the replicas (created with sdxl_*_create_empty: identical arena layout)
 * receive rank `root`'s packed weights.  Schedule: scatter of world equal pieces over the root's links + in-place all-gather
 * + a small tail broadcast (sdxl_bcast_plan describes it; no collective runs inside the sampling loop). */
typedef struct sdxl_comm sdxl_comm;
int sdxl_comm_unique_id(void* id_out_128);
int sdxl_comm_create(int device_id, int rank, int world, const void* id_128, sdxl_comm** out);
void sdxl_comm_destroy(sdxl_comm* c);
int sdxl_bcast_buffer(sdxl_comm* c, void* stream, void* base_dev, size_t bytes, int root);
int sdxl_unet_bcast_weights(sdxl_comm* c, sdxl_unet* u, int root);
int sdxl_vae_bcast_weights(sdxl_comm* c, sdxl_vae* v, int root);
int sdxl_clip_bcast_weights(sdxl_comm* c, sdxl_clip* k, int root);
/* the schedule as data: this rank's piece [piece_off, +piece_len) and the common tail [tail_off, +tail_len) of `bytes` */
int sdxl_bcast_plan(size_t bytes, int world, int rank, size_t* piece_off, size_t* piece_len, size_t* tail_off, size_t* tail_len);

/* ---- measurement: one eager UNet forward of the current plan/context with hipEvents around every launch, summed per
 * kernel class (index: 0 implicit-GEMM conv/linear, 1 fused attention, 2 GroupNorm, 3 LayerNorm, 4 other); arrays of 5 */
int sdxl_unet_profile(sdxl_unet* u, void* stream, int B, int H, int W, float class_ms[5], int class_launches[5],
                      double class_flops[5]);
/* the same eager chain without the per-launch events, one event pair around the whole forward (best of three): calibrates the event overhead
 * the class times of sdxl_unet_profile carry -- (sum of class_ms - *ms_out) / launches */
int sdxl_unet_eager_forward_ms(sdxl_unet* u, void* stream, int B, int H, int W, float* ms_out);
/* times the implicit-GEMM kernel alone (conv ksize x ksize, pad ksize/2, stride 1; ksize = 1 -> linear over B*H*W rows)
 * on seeded random f16 data; avg_ms = mean launch duration over `iters` back-to-back launches (hipEvents) */
int sdxl_bench_igemm(sdxl_ctx* ctx, void* stream, int B, int H, int W, int Cin, int Cout, int ksize, int geglu, int iters,
                     float* avg_ms);
/* times the fused attention kernel alone (head dim 64, f16) on seeded random data: B*H heads, Nq queries, Nk keys */
int sdxl_bench_attention(sdxl_ctx* ctx, void* stream, int B, int H, int Nq, int Nk, int iters, float* avg_ms);
/* benchmarking / debugging knobs.  "igemm_variant": -1 generic kernel only, 0 auto, > 0 forced fast-path tile / pipeline
 * (table in csrc/select.cpp); "attn_variant": -1 generic, 0 auto, 1/2/4/6 forced f16 kernels, 7/8 forced mixed block sizes,
 * 9 = auto without them (csrc/attention.hip);
 * "igemm_wreg": 0 = the auto selection never picks the weights-in-registers GEMM (csrc/igemm_wreg.hip; A/B, default 1), forced by
 * "igemm_variant" 60 / 62 (96 / 64 rows per tile); "igemm_epilogue_staged", "hl_weights_exact": A/B knobs of the epilogue form / the
 * two-MFMA loop of exact-f16 split-operand weights;
 * "wreg_xattn": 0 = the fused query projection + cross-attention of the f16 engine stays on the pipe kernels instead of the weights-in-registers
 *   GEMM with the attention behind its partial-sum exchange (csrc/igemm_wreg.hip, XA instantiation; A/B, default 1; the two sum k in different
 *   orders, so the results differ at rounding level; a UNet picks it up on its next forward, its weight-warming schedule when it is next recorded);
 * "xattn_long": 0 = contexts of more than 96 keys (prompts of two to four 77-token chunks) keep projection + attention kernel instead of the long form of
 *   the fused launch (csrc/igemm_common.h xattn_unit_long: 96-key blocks, online softmax; A/B, default 1; results differ at rounding level); read when a
 *   context is set (sdxl_unet_forward, the trajectory calls), so a UNet picks it up with its next context and re-captures its graph;
 * "igemm_warm": 0 = no weight-warming workgroups (spare workgroups of a weights-in-registers launch read a later GEMM's weights into the
 * Infinity Cache; results unchanged; A/B, default 1; a UNet picks it up on its next forward);
 * "attn_xsplit": 0 = the self-attention of the 32^2 level never runs 1/5 of its heads as two half-key blocks per 64 queries merged across
 * workgroups (csrc/attention.hip, attn_d64_mix_kernel level 2; A/B, default 1);
 * "splitk_wt": 0 = split-K slabs published by plain stores + an agent-scope release instead of write-through stores (A/B, default 1);
 * "hl_tile96": bit set of the extra tiles of the split-operand GEMMs (A/B; results unchanged): 1 = 96x128 for the M = 2048 x N = 1280 linears, 2 = ... for
 *   3x3 convolutions too, 4 = 4-wave 128x160 for widths that are multiples of 160 but not of 128, 8 = 128x160 wherever the cost model prefers it, 16 = in-launch split-K (3 slices) for the K >= 10240 convolutions of the 32^2 level (default 29);
 * "mix_classes": overrides the f16 classes of SDXL_DTYPE_F32_SPLIT_MIX* models built afterwards (1 = self-attention, 2 = GEGLU projection, 4 = QKV projection,
 *   8 = FF-out, 16 = self-attention out-projection, 32 = cross-attention out-projection, 64 = with 32: the cross-attention and its query projection as the f16
 *   engine's fused launch on an f16 copy of the context K / V -- measured 27.7 against 29.9 ms per step at 0.0195 of the 0.0212 bound, in no mode; -1 = the mode's own);
 *   A/B and bisecting (environment SDXL_NAN_CHECK=1 makes eager forwards report the first GEMM with a non-finite output on stderr);
 * "hl_demote": bit set of GEMM classes (csrc/engine.h DemoteClass) that a SDXL_DTYPE_F32_SPLIT UNet runs on operands with zero lo halves --
 *   the f16 engine's operand rounding class by class on the split engine's kernels: the precision-frontier instrument
 *   (tools/precision_frontier.py, profiles/r05_precision_frontier.json); takes effect at the next set_context / trajectory; default 0;
 * "upsample_fold": 0 = the nearest-2x upsample convolutions (f16 UNet, split-operand VAE decoder, sdxl_conv2d_upsample_folded) keep the 3x3 weights and the
 *   index >> 1 gather instead of the four-phase launch on folded weights (A/B and tests; results differ by the fold's weight rounding; read per launch, a
 *   captured UNet plan keeps what it recorded; default 1);
 * "igemm_unrolled": 0 = auto selection launches the rolled k-loop kernels (A/B; default 1);
 * "split_cfg": 1 = a batch-2 UNet::forward runs its two entries as two concurrent batch-1 chains (bit-identical results);
 * "split_offset": GEMM launches of the first chain before the second is released; "no_cfg": base model without the
 * unconditional branch (measurement only -- NOT the reference's semantics) */
int sdxl_debug_set(const char* key, int value);
/* host logic of the weight-warming schedule on a synthetic launch sequence (no device needed; tests): bytes[j] / host[j] = what entry j reads and
 * whether its kernel can carry warming workgroups; warmed_by[j] receives the index of the entry that warms j, -1 if nobody does */
int sdxl_debug_warm_schedule(int n, const unsigned* bytes, const unsigned char* host, int* warmed_by);
/* the weight fold of the upsample convolutions on HOST arrays (no device needed; tests): weight [cout][cin][3][3] -> out [4][cout][cin][2][2], phase
 * 2a + b of output pixel (2i + a, 2j + b), W_ab[dy][dx] = the taps of row set R_a(dy) x column set R_b(dx) summed in fp32, ky major, kx minor
 * (R_0(0) = {0}, R_0(1) = {1, 2}, R_1(0) = {0, 1}, R_1(1) = {2}) */
int sdxl_debug_upsample_fold(const float* weight, int cout, int cin, float* out);
/* the layout pass of a model's weight arena (no device needed; tests): *bytes receives what the model's weight arena holds -- sdxl_*_weight_arena of the
 * created model, the size of its weight broadcast.  Exactly one of unet / vae / clip is non-NULL.  option: UNet -- the MixClass bits in force, -1 =
 * the dtype's own (a model created on parameters that are not f16 values falls back to other classes: pass what sdxl_unet_mix_classes reports);
 * VAE -- 0 = decoder only, 1 = with the encoder; CLIP -- 0 */
int sdxl_debug_weight_layout(const sdxl_unet_config* unet, const sdxl_vae_config* vae, const sdxl_clip_config* clip, int dtype, int option, size_t* bytes);
/* the kernel selection on a described launch (no device needed, no process-wide state read or written; tests): which kernel instantiation, grid and LDS
 * bytes a GEMM / a head-dim-64 attention call with these integer fields, optional operands and knob values would launch.  Optional operands are named by
 * the SDXL_SEL_* bits of `present`; `misaligned` != 0 puts every operand 8 bytes off a 16-byte boundary.  A status != 0 (text in sdxl_last_error())
 * reports a launch the selection refuses.  dtypes: 0 fp32, 1 f16, 2 split-operand HL16 (engine-internal numbering). */
enum {
  SDXL_SEL_WF = 1 << 0, SDXL_SEL_R = 1 << 1, SDXL_SEL_EBIAS = 1 << 2, SDXL_SEL_STAT_OUT = 1 << 3, SDXL_SEL_LN_STAT = 1 << 4, SDXL_SEL_GN_PART = 1 << 5,
  SDXL_SEL_SHADOW = 1 << 6, SDXL_SEL_XA_K = 1 << 7, SDXL_SEL_XA_K_LO = 1 << 8, SDXL_SEL_ACC_SCALE = 1 << 9, SDXL_SEL_SPLITK_WS = 1 << 10,
  SDXL_SEL_XSPLIT_WS = 1 << 11, SDXL_SEL_MASK = 1 << 12, SDXL_SEL_WARM = 1 << 13
};
typedef struct sdxl_select_knobs {      /* the sdxl_debug_set keys of the same names; zero_page: the device's zero page exists (after sdxl_ctx_create) */
  int igemm_variant, igemm_wreg, wreg_xattn, hl_tile96, igemm_tsw, igemm_unrolled, wide_db, attn_variant, attn_xsplit, zero_page;
} sdxl_select_knobs;
typedef struct sdxl_igemm_case {
  int batch, rows_per_entry;            /* M = batch * rows_per_entry output rows (rows_per_entry = Hout * Wout, square) */
  int N, cin, ksize, stride, up;        /* K = ksize^2 * cin (Kpad: up to the k-tile); pad = ksize / 2 */
  int act, n_split;                     /* n_split < 0: none */
  int a_dt, c_dt, compute_dt;
  int xa_nctx, shadow_lo_sign;          /* sign of the shadow's lo scale (-1, 0, 1) */
  unsigned present; int misaligned;
} sdxl_igemm_case;
typedef struct sdxl_igemm_choice {      /* csrc/kernels.h IgemmChoice */
  int family, bm, bn, ns, wgm, nw, elem, a_elem, xa, xh, tsw, s2, splitk, mode, db, measure, grid, block, lds;
  int gn_part_ok, wreg_selected, wreg_xattn_selected;      /* what the predicates of the same rules answer for this launch */
} sdxl_igemm_choice;
int sdxl_debug_igemm_select(const sdxl_igemm_case* c, const sdxl_select_knobs* knobs, sdxl_igemm_choice* out);
typedef struct sdxl_attn_case { int B, H, Nq, Nk, dt; unsigned present; int misaligned; } sdxl_attn_case;
typedef struct sdxl_attn_choice { int kernel, mix, big_heads, ns, elem, ko, grid_x, grid_y, block, lds; } sdxl_attn_choice;      /* csrc/kernels.h AttnChoice */
int sdxl_debug_attn_select(const sdxl_attn_case* c, const sdxl_select_knobs* knobs, sdxl_attn_choice* out);

/* ---- single-op entry points used by the parity tests (same kernels the models run) */
/* GroupNorm::forward (groupnorm/mod.rs:52-73) on NCHW fp32 [B,C,H,W]; silu!=0 fuses SILU::forward (silu.rs:14-16) */
int sdxl_group_norm(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, int B, int C,
                    int HW, int n_group, float eps, int silu, int dtype, float* out);
/* LayerNorm::forward (layernorm/mod.rs:34-40) on [rows,C] */
int sdxl_layer_norm(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, int rows, int C,
                    float eps, int dtype, float* out);
/* burn Conv2d on NCHW fp32: weight [Cout,Cin,k,k], bias [Cout]; upsample!=0 applies nearest-2x first (unet/mod.rs:744-750) */
int sdxl_conv2d(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, int B, int Cin,
                int H, int W, int Cout, int ksize, int stride, int pad, int upsample, int dtype, float* out);
/* nearest-2x upsample + Conv2d 3x3 pad 1 (Upsample::forward, unet/mod.rs:742-752; the decoder's upsampler) as the f16 UNet and the split-operand VAE
 * decoder run it: the upsample folded into the weights -- four 2x2-tap phase matrices, summed in fp32 and then packed (one more weight rounding in the
 * f16 engine than sdxl_conv2d(..., upsample = 1), which keeps the 3x3 weights) -- and one phase-ordered launch.  dtype: SDXL_DTYPE_F16 (Cin % 64 == 0) or
 * SDXL_DTYPE_F32_SPLIT (Cin % 32 == 0).  Shapes without such a launch (H * W % 128 != 0) and sdxl_debug_set("upsample_fold", 0) take the gather form on
 * the 3x3 weights; *folded (may be NULL) reports which ran.  x [B,Cin,H,W], weight [Cout,Cin,3,3], out [B,Cout,2H,2W], fp32 device tensors. */
int sdxl_conv2d_upsample_folded(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, int B, int Cin, int H, int W,
                                int Cout, int dtype, int* folded, float* out);
/* burn nn::Linear: y = x[M,K] @ W[K,N] + b; geglu!=0 returns x_half * gelu_erf(gate_half) (unet/mod.rs:942-956) */
int sdxl_linear(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, int M, int K, int N,
                int geglu, int dtype, float* out);
/* The small-M linear of the UNet's conditioning path (time / label embedding MLPs, unet/mod.rs:458-468, and the ResBlocks' lin_embed(silu(emb)),
 * :1088-1089), on the GEMV kernel and launcher UNet::forward runs:  out[b] = silu_out?(silu_in?(x[b]) @ W[K,N] + bias) + yadd[b].
 * x [Bm,K], weight [K,N] (in,out), bias [N] or NULL, yadd [Bm,N] or NULL, out [Bm,N]; dense fp32 device tensors, any Bm >= 1 (the launcher splits the
 * rows over launches of at most 8 rows and 64 KiB of staged inputs; K beyond one row of that is an error).  dtype: SDXL_DTYPE_F32 (fp32 weights),
 * SDXL_DTYPE_F16 (f16 weights), SDXL_DTYPE_F32_SPLIT (fp32 weights: what a split-operand UNet packs for this kernel); accumulation is fp32 in all. */
int sdxl_gemv(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, const float* yadd, int Bm, int K, int N,
              int silu_in, int silu_out, int dtype, float* out);
/* timestep_embedding (unet/mod.rs:21-39) of n fp32 device timesteps: out [n,dim] = [cos(t f) | sin(t f)], f_j = exp(j * -ln(10000) / (dim / 2));
 * dim even */
int sdxl_timestep_embedding(sdxl_ctx* ctx, void* stream, const float* t, int n, int dim, float* out);
/* The two blocks of the autoencoder on their own, through the code the LatentDecoder's decoder and encoder run (parity tests).  NCHW fp32 device tensors
 * in and out; convolution weights [Cout,Cin,k,k], biases [Cout] or NULL; dtype as sdxl_vae_create takes it, one of SDXL_DTYPE_F32, SDXL_DTYPE_F16,
 * SDXL_DTYPE_F32_SPLIT (channel counts % 32 == 0), mapped to compute / stream dtypes as a VAE handle maps it; channel counts divisible by n_group and by 8.
 * sdxl_vae_attn_block: ConvSelfAttentionBlock::forward (autoencoder/mod.rs:550-586): out = x + proj_out(attention(q, k, v of GroupNorm(x))), one head of C
 *   channels, softmax(q k^T / sqrt(C)); wq / wk / wv / wo [C,C,1,1].  C a multiple of the k-tile (64 in f16, else 32).
 * sdxl_vae_res_block: ResnetBlock::forward (:500-516): out = shortcut(x) + conv2(silu(GN2(conv1(silu(GN1(x)))))), w1 [Cout,Cin,3,3], w2 [Cout,Cout,3,3],
 *   w_nin [Cout,Cin,1,1] (NULL only where Cin == Cout: the shortcut is x itself). */
int sdxl_vae_attn_block(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, float eps, const float* wq, const float* bq,
                        const float* wk, const float* bk, const float* wv, const float* bv, const float* wo, const float* bo, int B, int C, int H, int W,
                        int n_group, int dtype, float* out);
int sdxl_vae_res_block(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma1, const float* beta1, float eps1, const float* w1, const float* b1,
                       const float* gamma2, const float* beta2, float eps2, const float* w2, const float* b2, const float* w_nin, const float* b_nin, int B,
                       int Cin, int Cout, int H, int W, int n_group, int dtype, float* out);
/* One entry of a UNet's block plan on its own, through the code sdxl_unet_forward runs for it (parity tests): section 0 = input_blocks[index] (Conv, Res,
 * Res + SpatialTransformer, Down), 1 = the middle block (res1, transformer, res2; index 0), 2 = output_blocks[index] (Res, optionally + SpatialTransformer,
 * optionally + the upsample convolution), 3 = norm_out + SiLU + conv_out (index 0).  NCHW fp32 device tensors: x [B,c_in,h,w] at the entry's OWN resolution
 * (c_in: the concat width for output entries), emb [B,4*model_channels] = t_emb + l_emb (what every ResBlock's lin_embed(silu(emb)) consumes), context
 * [B,n_ctx,context_dim], out [B,c_out,h_out,w_out] (h_out = (h - 1) / 2 + 1 for a Down entry, 2h behind an upsample convolution, else h).
 * The entry is run as inside a forward of the top-level size its level implies (h, w times 2^level): x is laid out with the row stride its source has
 * there (the previous entry's slice of a concat buffer; the whole buffer for output entries), the result is written at the row stride and column offset
 * its destination has there, the time-embedding bias is the entry's slice of the one GEMV over all ResBlocks, the cross-attention caches are the entry's
 * own among all transformers'.  The per-handle options (sdxl_unet_set_fused_cross_attention, sdxl_unet_set_gn_from_producer) apply.
 * out_shape (may be NULL) receives {B, c_out, h_out, w_out}; out == NULL: only that, nothing is launched.
 * SDXL_ERR_INVALID, nothing launched: an index outside the plan, c_in not the entry's width, a size no forward has at that level (top-level height and
 * width must be divisible by 2^(levels-1)), B outside 1..8, a top-level height or width above 256, a NULL x / emb / context with out != NULL.
 * Replaces the handle's context and leaves no label embedding: sdxl_unet_forward sets its own again; a Diffuser whose UNet handle ran an entry refuses
 * (SDXL_ERR_RUNTIME) to step until its conditioning is set again. */
int sdxl_unet_block(sdxl_unet* u, void* stream, int section, int index, const float* x, const float* emb, const float* context, int B, int c_in, int h,
                    int w, int n_ctx, float* out, int64_t out_shape[4]);
/* ---- ControlNet skip residuals (Zhang et al. 2023; sgm ControlledUnetModel, diffusers down_block_additional_residuals / mid_block_additional_residual).
 * A controlled forward runs the encoder unchanged, then  h = middle(h) + s r_mid  and every output block concatenates  hs.pop() + s r.pop().
 * The residual tensors of a UNet are, in this order: one per input entry (the entry's output shape), then the middle block's.
 * sdxl_unet_skip_count: their number, input entries + 1 (-1 with sdxl_last_error on a bad config).  sdxl_unet_skip_shape: {C, h, w} of tensor `index`
 * for an H x W latent.  Both are host logic only.  SDXL_ERR_INVALID: an index outside 0 .. count - 1, H or W not a positive multiple of 2^(levels-1). */
int sdxl_unet_skip_count(const sdxl_unet_config* cfg);
int sdxl_unet_skip_shape(const sdxl_unet_config* cfg, int index, int H, int W, int64_t chw[3]);
/* sdxl_unet_forward with residuals given by the caller: `residuals` holds all sdxl_unet_skip_count tensors back to back, each NCHW fp32
 * [B,C,h,w] (device).  They are converted once into staging buffers of the handle in its stream dtype (fp32, or f16 for SDXL_DTYPE_F16), and ONE launch
 * behind the middle block adds scale times each of them into the tensor the decoder reads (sdxl_skip_residual_add's kernel), in place.  The scale
 * travels in device memory: calling again with another scale, or other residuals, replays the captured graph.  The handle keeps the residuals
 * attached for later calls of this entry; residuals == NULL, or sdxl_unet_forward, detaches them (attaching and detaching re-capture the graph) and runs
 * exactly the launches of a handle that never had any.
 * SDXL_ERR_INVALID, nothing launched, the handle as it was: a non-finite scale; a handle with sdxl_unet_set_split_cfg enabled (split CFG and
 * skip residuals cannot be combined); SDXL_DTYPE_F16_F32RES, the SDXL_DTYPE_F32_SPLIT_MIX* modes and SDXL_DTYPE_F32_SPLIT_F16W (no test covers them). */
int sdxl_unet_forward_residuals(sdxl_unet* u, void* stream, const float* x, const int32_t* timesteps, const float* context, const float* label,
                                int B, int H, int W, int n_ctx, const float* residuals, float scale, float* out);
/* The per-step add on caller buffers: for each of the n_segments (1 .. 16) segments i, rows[i] rows of C[i] channels,
 *   dst[i][r * dst_ld[i] + c] = round(fma(*scale_dev, src[i][r * C[i] + c], dst[i][r * dst_ld[i] + c]))      (fp32 fma, one rounding to the dtype)
 * in ONE launch, in place.  dst / src are device buffers of the dtype (SDXL_DTYPE_F32: float, SDXL_DTYPE_F16: IEEE f16); src rows are dense, dst rows
 * dst_ld[i] elements apart (a column slice of a wider buffer); scale_dev is a device float.  Segments must not overlap.
 * SDXL_ERR_INVALID, nothing launched: n_segments outside 1 .. 16, another dtype, rows < 0, C <= 0 or C % 8 != 0, dst_ld < C, a dst / src pointer or a
 * dst row pitch that is not 16-byte aligned. */
int sdxl_skip_residual_add(sdxl_ctx* ctx, void* stream, int n_segments, void* const* dst, const int64_t* dst_ld, const void* const* src,
                           const int64_t* rows, const int32_t* C, const float* scale_dev, int dtype);
/* ---- ControlNet: a second copy of the controlled UNet's encoder (embeddings, input entries, middle block: the UNet's own code, caches and packing),
 * a hint embedder, one 1x1 convolution per residual tensor.  cfg.unet is the configuration of the UNet being controlled.
 * Parameters (sdxl_controlnet_param_spec, conventions of sdxl_unet_param_spec): the UNet's lin1/lin2_time_embed, lin1/lin2_label_embed, input_blocks.{i},
 * middle_block.{res1,transformer,res2} under their own names and in their order; input_hint_block.{0..7}: 3x3 pad-1 convolutions hint_in -> hc0 -> hc0
 * -> hc1 -> hc1 -> hc2 -> hc2 -> hc3 -> model_channels, numbers 2, 4 and 6 with stride 2, SiLU behind each of the first seven; zero_convs.{i}: 1x1, c_i ->
 * c_i for every input entry i; middle_block_out: 1x1.  (Checkpoints initialise zero_convs to zero; the synthetic ones are not zero.)
 * Control forward: g = input_hint_block(hint), h = x; per input entry i: h = input_blocks[i](h, emb, context), h += g behind entry 0,
 * r_i = zero_convs[i](h); then r_mid = middle_block_out(middle_block(h)).  hint is [n, hint_in, 8H, 8W] fp32 for an H x W latent; g does not depend
 * on the timestep and is computed once per hint, never per step. */
typedef struct sdxl_controlnet sdxl_controlnet;
typedef struct {
  sdxl_unet_config unet;
  int32_t hint_in_channels;   /* 3 */
  int32_t hint_channels[4];   /* 16, 32, 96, 256 */
} sdxl_controlnet_config;
void sdxl_controlnet_config_default(const sdxl_unet_config* unet, sdxl_controlnet_config* cfg);
int sdxl_controlnet_param_count(const sdxl_controlnet_config* cfg);      /* host logic only; -1 with sdxl_last_error on a bad config */
int sdxl_controlnet_param_spec(const sdxl_controlnet_config* cfg, int index, const char** name, int* ndim, int64_t shape[4], int* kind,
                               float* synth_scale, float* synth_mean);
/* dtype: SDXL_DTYPE_F32, SDXL_DTYPE_F16 or SDXL_DTYPE_F32_SPLIT -- every other mode is refused by name (SDXL_ERR_INVALID), as is a refiner
 * configuration (unet.is_refiner != 0: there is no refiner ControlNet).  */
int sdxl_controlnet_create(sdxl_ctx* ctx, const sdxl_controlnet_config* cfg, int dtype, const float* weights_flat, sdxl_controlnet** out);
int sdxl_controlnet_create_f16(sdxl_ctx* ctx, const sdxl_controlnet_config* cfg, int dtype, const uint16_t* weights_flat_f16, sdxl_controlnet** out);
int sdxl_controlnet_create_synthetic(sdxl_ctx* ctx, const sdxl_controlnet_config* cfg, int dtype, uint64_t seed, sdxl_controlnet** out);
void sdxl_controlnet_destroy(sdxl_controlnet* c);
/* the hint embedder alone: hint [n, hint_in, H8, W8] -> out [n, model_channels, H8 / 8, W8 / 8], fp32 device tensors */
int sdxl_controlnet_embed_hint(sdxl_controlnet* c, void* stream, const float* hint, int n, int H8, int W8, float* out);
/* the control forward, reference-shaped like sdxl_unet_forward: x [B,in,H,W], timesteps int32 [B] (device), context [B,n_ctx,ctx_dim], label [B,adm],
 * hint [B,hint_in,8H,8W]; residuals_out receives all sdxl_unet_skip_count tensors back to back, each NCHW fp32 [B,C,h,w] -- the layout
 * sdxl_unet_forward_residuals takes */
int sdxl_controlnet_forward(sdxl_controlnet* c, void* stream, const float* x, const int32_t* timesteps, const float* context, const float* label,
                            const float* hint, int B, int H, int W, int n_ctx, float* residuals_out);
/* The per-step add as a trajectory needs it: sdxl_skip_residual_add with one scale per batch entry and iteration.  The scale of element (r, c) of
 * segment i is  s = scales_dev[*step_idx_dev * 8 + b],  b = r / (rows[i] / B)  the batch entry of row r: scales_dev is a device table of rows of 8
 * floats (a trajectory's has iterations + 1 rows), step_idx_dev a device int32 naming the row.  Where s != 0 the arithmetic is sdxl_skip_residual_add's;
 * where s == 0 the element is neither read from src nor written to dst (src may hold anything there, NaN included).
 * SDXL_ERR_INVALID, nothing launched: what sdxl_skip_residual_add refuses, B outside 1 .. 8, a rows[i] that is no multiple of B. */
int sdxl_skip_residual_add_steps(sdxl_ctx* ctx, void* stream, int n_segments, void* const* dst, const int64_t* dst_ld, const void* const* src,
                                 const int64_t* rows, const int32_t* C, int B, const float* scales_dev, const int32_t* step_idx_dev, int dtype);
/* ---- Control options: how a control net's residuals enter a trajectory, as the scale of every iteration i (timestep t_i) and batch entry b
 *   s(i, b) = (t_lo <= t_i <= t_hi) ? (n_scales ? scales[b mod n] : scale) : 0,     and 0 for the unconditional entries b >= n where cond_only is set
 * (entries 0 .. n-1 are the conditional ones, n .. 2n-1 the unconditional ones of the CFG pair; t_lo / t_hi are diffusers' control_guidance_start /
 * _end as timesteps) -- rows of the table sdxl_skip_residual_add_steps reads.  sdxl_control_scale_table builds such a table from them.  The
 * Diffuser's trajectories do not take a control net yet. */
typedef struct {
  float   scale;       /* conditioning scale of every entry (default 1) */
  int32_t n_scales;    /* 0, or cond.n */
  float   scales[8];   /* per-entry scales, replace `scale` */
  int32_t t_lo, t_hi;  /* control is active on iterations whose timestep t has t_lo <= t <= t_hi; default 0 .. INT32_MAX */
  int32_t cond_only;   /* != 0: residuals for the conditional entries only (default 0) */
} sdxl_control;
void sdxl_control_default(sdxl_control* c);
/* host logic only (no device).  SDXL_ERR_INVALID with the reason in sdxl_last_error: a non-finite scale; n_scales outside 0..8; t_lo < 0 or
 * t_lo > t_hi; cond_only with single_branch != 0 (one branch, as under SDXL_GUIDANCE_OFF, has no unconditional entries). */
int sdxl_control_check(const sdxl_control* c, int single_branch);
/* host logic only (no device): the scales of one control net over a trajectory.  timesteps: the iters timesteps t_i of the schedule, in order; n: cond.n;
 * out: [iters + 1][8] floats,  out[i][b] = s(i, b)  for the entries b of the batch (n with single_branch != 0, else 2 n) and 0 behind them; row `iters`
 * is all zeros (the row a trajectory's step index rests on after its last iteration).
 * SDXL_ERR_INVALID, out untouched: what sdxl_control_check refuses; n < 1 or a batch above 8; n_scales neither 0 nor n; iters < 0; a null pointer. */
int sdxl_control_scale_table(const sdxl_control* c, int n, int single_branch, const int32_t* timesteps, int iters, float* out);
/* The per-step add with K sources per destination (K control nets on one UNet), in ONE launch with one rounding: src holds n_segments x K pointers,
 * src[i * K + k] the dense [rows[i]][C[i]] source k of segment i; scales_dev is a device table of rows of K x 8 floats, and source k of element (r, c)
 * of segment i has the scale  s_k = scales_dev[(*step_idx_dev * K + k) * 8 + b],  b = r / (rows[i] / B).  Per element, in fp32:
 *   v = dst;  for k = 0 .. K-1 in order, where s_k != 0:  v = fma(s_k, src_k, v);   dst = round(v) where any s_k != 0.
 * A source whose own scale is 0 is not read, whatever the others' scales: it may hold NaN, or end before row r (a control net that ran on the
 * conditional entries alone holds the first rows[i] / B * n rows).  An element all of whose scales are 0 is not written.  K == 1 gives the bits of
 * sdxl_skip_residual_add_steps.
 * SDXL_ERR_INVALID, nothing launched: what sdxl_skip_residual_add_steps refuses (for every one of the K sources), K outside 1 .. SDXL_MAX_CONTROLS. */
#define SDXL_MAX_CONTROLS 4
int sdxl_skip_residual_add_steps_multi(sdxl_ctx* ctx, void* stream, int n_segments, void* const* dst, const int64_t* dst_ld, const void* const* src, int K,
                                       const int64_t* rows, const int32_t* C, int B, const float* scales_dev, const int32_t* step_idx_dev, int dtype);
/* LayerNorm::forward (layernorm/mod.rs:34-49) followed by nn::Linear, as TransformerBlock::forward pairs them
 * (unet/mod.rs:885-891): y = LN(x[M,K]; gamma, beta, eps) @ W[K,N] + b (bias may be NULL), optional GEGLU.  Runs the path
 * the UNet runs in that dtype: SDXL_DTYPE_F16 = LayerNorm folded into the GEMM (row statistics from the producer's
 * epilogue), otherwise the stand-alone LayerNorm kernel.  K % 64 == 0. */
int sdxl_layer_norm_linear(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, float eps,
                           const float* weight, const float* bias, int M, int K, int N, int geglu, int dtype, float* out);

/* LayerNorm -> attn2 query projection (no bias) -> qkv_attention over the already projected context, 64 channels per head:
 * SpatialTransformer block attn2 up to its output projection (src/model/unet/mod.rs:731-795, attention via backend.rs:88-128).
 * x [B,Nq,C], wq [C,C] (in,out), k,v [B,Nk,C], out [B,Nq,C]; fp32 device tensors, f16 engine arithmetic.
 * fused != 0: ONE launch, the attention runs in the projection's epilogue (needs Nq % 64 == 0).  fused == 1: Nk <= 96 at any C, and
 *   97 <= Nk <= 384 where C % 128 == 0 (the weights-in-registers form walks the context in 96-key blocks); other widths above 96 keys
 *   and Nk > 384 return "fused cross-attention: unsupported shape" and launch nothing -- they are never run un-fused silently.
 *   fused == 2 (split precision): Nk <= 96;
 * fused == 0: projection + attention kernel. */
int sdxl_ln_query_cross_attention(sdxl_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta, float eps,
                                  const float* wq, const float* k, const float* v, int B, int Nq, int Nk, int C, int fused,
                                  float* out);

/* forms of a transformer projection on the split-operand UNet (SDXL_DTYPE_F32_SPLIT_MIX* / _F16W): NATIVE = (hi, lo) operands, three MFMAs
 * per product; F16 = f16 activations x f16 weights; F16_WHILO = f16 activations x (hi | lo) weight halves along a doubled K; F16_AHILO = (hi | lo)
 * activation halves x f16 weights; X2 = HL16 activations x the f16 weight packed twice in the HL16 interleave */
enum { SDXL_FORM_NATIVE = 0, SDXL_FORM_F16 = 1, SDXL_FORM_F16_WHILO = 2, SDXL_FORM_F16_AHILO = 3, SDXL_FORM_X2 = 4 };
/* the LayerNorm-fed projections of a transformer block: attn1 QKV (fused along N), attn2 query, the GEGLU projection */
enum { SDXL_PROJ_QKV = 0, SDXL_PROJ_QUERY = 1, SDXL_PROJ_GEGLU = 2 };
/* One LayerNorm-fed projection of a split-operand UNet transformer block in a given form, run by the UNet's own code.  B entries of rows_per_entry rows
 * (M = B x rows_per_entry), C channels; fp32 device tensors.
 *   producer (producer_form >= 0: SDXL_FORM_NATIVE, _F16 or _X2): t = r + a[M,Kp] @ wp[Kp,C] + bp, the out-projection / FF-out that writes the residual
 *   stream; producer_form < 0: t = r (a, wp, bp unused).
 *   consumer: LayerNorm(t; gamma, beta, eps) @ w[C,N] + b (b may be NULL), GEGLU for SDXL_PROJ_GEGLU (out [M, N/2], else [M, N]).
 *   shadow != 0: the producer is asked for the LayerNorm shadow (MIX_LN_SHADOW) and the consumer runs its shadow twin where the producer's kernel left
 *   it, otherwise the LayerNorm launch and the plain form.  *shadow_taken (may be NULL): whether the shadow was taken.  t_out (may be NULL): t.
 * Arguments outside what the form supports (C or N % 32 != 0, X2 with N % 128 != 0, AHILO / X2 on weights that are not f16 values, a shadow with
 * C % 64 != 0 or without an F16 / X2 producer, ...) return SDXL_ERR_INVALID. */
int sdxl_transformer_projection(sdxl_ctx* ctx, void* stream, int B, int rows_per_entry, int C, const float* a, const float* wp, const float* bp,
                                const float* r, int Kp, int producer_form, const float* gamma, const float* beta, float eps, const float* w,
                                const float* b, int N, int proj, int form, int shadow, float* t_out, float* out, int* shadow_taken);

/* conv3x3 (pad 1, optional residual) -> GroupNorm (+SiLU): the conv -> norm pairs of ResBlock::forward (src/model/unet/mod.rs:
 * 1082-1106) and of the SpatialTransformer entry (:820-845), f16 engine arithmetic.  x [B,Cin,H,W], weight [Cout,Cin,3,3],
 * residual / out [B,Cout,H,W]; fp32 device tensors.  fused != 0: the convolution's epilogue leaves the GroupNorm statistics
 * (no statistics pass); *fused_taken (may be NULL) reports whether the selected kernel could (256-row tiles, 64-column waves). */
int sdxl_conv2d_group_norm(sdxl_ctx* ctx, void* stream, const float* x, const float* weight, const float* bias, const float* residual,
                           const float* gamma, const float* beta, float eps, int B, int Cin, int H, int W, int Cout, int n_group,
                           int silu, int fused, int* fused_taken, float* out);

#ifdef __cplusplus
}
#endif
#endif /* SDXL_MI355_H */
