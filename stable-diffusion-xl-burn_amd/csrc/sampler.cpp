// DDIM (eta = 0) sampler with classifier-free guidance -- reference Diffuser (stablediffusion/mod.rs:308-542).
//
// What changes relative to the reference's loop, without changing its arithmetic:
//   * the CFG pair runs as ONE batch-2n UNet forward (cond entries [0,n), uncond [n,2n)) instead of two sequential
//     batch-n forwards (:523-537): weights stream from HBM once per step and every GEMM has 2x the rows to fill 256 CUs.
//     Per-sample ops (GroupNorm, attention, LayerNorm) never mix batch entries, so results equal two separate calls.
//   * alpha lookups (:407-412, two blocking device->host scalar reads per step in the reference) become a per-trajectory
//     coefficient table computed on the host in f64 and uploaded once; the step index lives on the device, so every
//     iteration is the same captured graph + one fused CFG/DDIM/inpaint kernel, with no host sync inside the loop.
//   * noise is an explicit input (the reference's generator is unseeded, gen_noise :378-388) with sigma = 0, or, in the
//     *_seeded calls, drawn on the device from one seed per batch entry: the initial latent by a fill kernel, the inpainting
//     blend (:463) and the gen_noise()*sigma term (:427, sigma from eta) in the registers of the per-step kernel.
//   * the update itself is a per-handle choice (set_solver): the reference's DDIM, or DPM-Solver++(2M) on the same schedule, same table
//     mechanism and same fused kernel position, with one more latent-sized buffer for the previous data prediction.
//   * how the pair becomes e is a per-handle choice too (set_guidance): the reference's one line by default; the conditional branch alone as a
//     batch-n forward; or per-entry scales, a timestep interval and CFG rescale, run by launch_guided_step in the per-step kernel's place with
//     two small launches in front of it where rescale is on.  A handle with default options launches what it always launched.
#include "engine.h"

#include <algorithm>
#include <cmath>

namespace sdxl {

std::vector<int> Diffuser::step_schedule(int n_steps, int step_start, int n_train) {
  // (0..n_train-step_start).rev().step_by(n_train / n_steps)   (:400-406); n_steps=30 -> 31 iterations
  SDXL_REQUIRE(n_steps >= 1 && n_steps <= n_train, "n_steps out of range");
  const int step = n_train / n_steps;
  std::vector<int> ts;
  for (int t = n_train - step_start - 1; t >= 0; t -= step) ts.push_back(t);
  return ts;
}

Diffuser::Diffuser(const UNetCfg& cfg, int compute_dt, int stream_dt, WeightSource& src, const float* alphas_host,
                   int n_train, hipStream_t st, int mix)
    : n_train_(n_train), is_refiner_(cfg.is_refiner) {
  unet_.reset(new UNet(cfg, compute_dt, stream_dt, src, st, mix));
  alphas_.resize(n_train);
  for (int i = 0; i < n_train; ++i) alphas_[i] = (double)alphas_host[i];   // get_alpha :485-492 (elem -> f64)
  SDXL_HIP(hipMalloc((void**)&step_idx_, sizeof(int)));
  SDXL_HIP(hipMalloc((void**)&t_dev_, 8 * sizeof(float)));
}
Diffuser::~Diffuser() {
  for (void* p : {(void*)latent_, (void*)noise_, (void*)hist_, (void*)table_, (void*)step_idx_, (void*)t_dev_, (void*)ctx_buf_, (void*)y_buf_,
                  (void*)active_, (void*)moments_, (void*)factors_})
    if (p) (void)hipFree(p);
}

// sigma (:423 pins it to 0.0): standard DDIM eta; ap = 1 on the last iteration, so nothing is drawn there
static void ddim_terms(double a, double ap, double eta, double& sqrt_ap, double& sqrt_1map, double& sigma) {
  sigma = eta == 0.0 ? 0.0 : eta * std::sqrt((1.0 - ap) / (1.0 - a)) * std::sqrt(1.0 - a / ap);
  sqrt_ap = std::sqrt(ap);
  sqrt_1map = std::sqrt(std::max(1.0 - ap - sigma * sigma, 0.0));
}

void Diffuser::set_solver(int solver) {
  SDXL_REQUIRE(solver == kSolverDdim || solver == kSolverDpmpp2M, "unknown solver");
  solver_ = solver;
}

const char* Diffuser::guidance_error(const Guidance& g, bool is_refiner) {
  if (g.mode != kGuidanceCfg && g.mode != kGuidanceOff) return "guidance: unknown mode (SDXL_GUIDANCE_CFG, SDXL_GUIDANCE_OFF)";
  if (!(g.rescale >= 0.f && g.rescale <= 1.f)) return "guidance: rescale must be a finite value in [0, 1]";
  if (g.n_scales < 0 || g.n_scales > kMaxSeeds) return "guidance: n_scales out of range (0..8)";
  for (int b = 0; b < g.n_scales; ++b)
    if (!std::isfinite(g.scales[b])) return "guidance: scales must be finite";
  if (g.t_lo < 0 || g.t_lo > g.t_hi) return "guidance: interval needs 0 <= t_lo <= t_hi";
  if (g.mode == kGuidanceOff && (g.rescale != 0.f || g.n_scales != 0 || g.t_lo != 0 || g.t_hi != 0x7fffffff))
    return "guidance: SDXL_GUIDANCE_OFF takes no rescale, scales or interval";
  if (is_refiner && !(g.plain() || g.mode == kGuidanceOff))
    return "guidance: a refiner handle has no unconditional branch (default options or SDXL_GUIDANCE_OFF only)";
  return nullptr;
}
void Diffuser::set_guidance(const Guidance& g) {
  const char* m = guidance_error(g, is_refiner_);
  SDXL_REQUIRE(m == nullptr, m ? m : "");
  guidance_ = g;
}

void Diffuser::solver_coefficients(const double* alphas, int n_train, int n_steps, int step_start, int solver, double eta, double* out) {
  SDXL_REQUIRE(solver == kSolverDdim || solver == kSolverDpmpp2M, "unknown solver");
  const std::vector<int> ts = step_schedule(n_steps, step_start, n_train);
  const int step_size = n_train / n_steps;
  double h_prev = 0.0;
  bool have_prev = false;       // false on iteration 0: no history, first order
  for (size_t i = 0; i < ts.size(); ++i) {
    const int t = ts[i];
    const double a = alphas[t];
    const double ap = t >= step_size ? alphas[t - step_size] : 1.0;
    SDXL_REQUIRE(a > 0.0 && a < 1.0 && ap > 0.0 && ap <= 1.0, "alphas_cumprod outside (0, 1)");
    const double alpha = std::sqrt(a), sigma = std::sqrt(1.0 - a);
    double* c = out + 4 * i;     // c_x, c_0, c_1, c_z
    if (solver == kSolverDdim) {
      double sqrt_ap, sqrt_1map, sigma_t;
      ddim_terms(a, ap, eta, sqrt_ap, sqrt_1map, sigma_t);
      c[0] = sqrt_1map / sigma; c[1] = sqrt_ap - sqrt_1map * alpha / sigma; c[2] = 0.0; c[3] = sigma_t;
      continue;
    }
    if (ap == 1.0) {             // h is infinite: the step lands on the data prediction
      c[0] = 0.0; c[1] = 1.0; c[2] = 0.0; c[3] = 0.0;
      have_prev = false;
      continue;
    }
    const double alpha_p = std::sqrt(ap), sigma_p = std::sqrt(1.0 - ap);
    const double h = std::log(alpha_p / sigma_p) - std::log(alpha / sigma);
    const double A = -std::expm1(-(1.0 + eta) * h);
    c[0] = (sigma_p / sigma) * std::exp(-eta * h);
    c[3] = sigma_p * std::sqrt(-std::expm1(-2.0 * eta * h));
    if (have_prev) {
      const double r = h_prev / h;
      c[1] = alpha_p * A * (1.0 + 1.0 / (2.0 * r));
      c[2] = -alpha_p * A / (2.0 * r);
    } else {
      c[1] = alpha_p * A;
      c[2] = 0.0;
    }
    h_prev = h;
    have_prev = true;
  }
}

#ifdef SDXL_MEASURE
bool g_debug_no_cfg = false;
#else
static constexpr bool g_debug_no_cfg = false;
#endif

static void ensure_latent(float*& buf, size_t& cap, size_t elems) {
  if (elems > cap) {
    if (buf) SDXL_HIP(hipFree(buf));
    SDXL_HIP(hipMalloc((void**)&buf, elems * sizeof(float)));
    cap = elems;
  }
}

void Diffuser::diffuse(float* latent, const Conditioning& c, int step_start, int n_steps, double cfg_scale,
                       const float* reference, const unsigned char* mask, const float* step_noise, hipStream_t s,
                       const uint64_t* seeds, double eta) {
  // diffuse_latent :390-432 / diffuse_latent_with_inpainting :434-483
  UNet& u = *unet_;
  const UNetCfg& uc = u.cfg();
  const Guidance& go = guidance_;
  // kGuidanceOff: conditional branch only, as for a refiner (debug knob: the same for concurrency experiments)
  const bool single = is_refiner_ || go.mode == kGuidanceOff || g_debug_no_cfg;
  const bool guided = !single && !go.plain();          // non-default options: the update launch is launch_guided_step
  const int n = c.n, B = single ? n : 2 * n;
  SDXL_REQUIRE(!guided || go.n_scales == 0 || go.n_scales == n, "guidance: n_scales differs from the batch (cond.n)");
  SDXL_REQUIRE(n >= 1 && B <= 8, "batch out of range");
  static_assert(kMaxSeeds >= 8, "one seed per batch entry");
  const int h = c.height / 8, w = c.width / 8, HW = h * w;
  const int ctx_dim = uc.context_dim, adm = uc.adm_in_channels;
  // --- contexts of the batched CFG pair (forward_diffuser :506-537)
  const float* ctx = is_refiner_ ? c.context_open_clip : c.context_full;
  const float* uctx = is_refiner_ ? c.unconditional_context_open_clip : c.unconditional_context_full;
  const float* y = is_refiner_ ? c.channel_context_refiner : c.channel_context;
  const float* uy = is_refiner_ ? c.unconditional_channel_context_refiner : c.unconditional_channel_context;
  SDXL_REQUIRE(ctx && y, "conditioning tensors missing");
  SDXL_REQUIRE(single || (uctx && uy), "unconditional conditioning tensors missing");
  const size_t ctx_elems = (size_t)c.n_ctx * ctx_dim;
  if ((size_t)B * ctx_elems > ctx_cap_) {
    if (ctx_buf_) SDXL_HIP(hipFree(ctx_buf_));
    SDXL_HIP(hipMalloc((void**)&ctx_buf_, (size_t)B * ctx_elems * sizeof(float)));
    ctx_cap_ = (size_t)B * ctx_elems;
  }
  if ((size_t)B * adm > y_cap_) {
    if (y_buf_) SDXL_HIP(hipFree(y_buf_));
    SDXL_HIP(hipMalloc((void**)&y_buf_, (size_t)B * adm * sizeof(float)));
    y_cap_ = (size_t)B * adm;
  }
  SDXL_HIP(hipMemcpyAsync(ctx_buf_, ctx, (size_t)n * ctx_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
  SDXL_HIP(hipMemcpyAsync(y_buf_, y, (size_t)n * adm * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (!single)
    for (int i = 0; i < n; ++i) {   // unconditional_context.unsqueeze().repeat(0, n_batch) :535-536
      SDXL_HIP(hipMemcpyAsync(ctx_buf_ + (size_t)(n + i) * ctx_elems, uctx, ctx_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
      SDXL_HIP(hipMemcpyAsync(y_buf_ + (size_t)(n + i) * adm, uy, adm * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  void* unet_in = u.unet_in(B, h, w);
  u.set_context(ctx_buf_, c.n_ctx, y_buf_, B, s);

  // --- coefficient table (host f64, exactly the reference's scalar arithmetic :407-414, :423-426)
  const std::vector<int> ts = step_schedule(n_steps, step_start, n_train_);
  const int iters = (int)ts.size();
  const int step_size = n_train_ / n_steps;
  std::vector<StepCoef> tab(iters + 1);
  std::vector<int> act(guided ? iters : 0);            // guidance interval: iteration i is active where t_lo <= t_i <= t_hi
  std::vector<double> c2m;
  if (solver_ == kSolverDpmpp2M) {
    c2m.resize((size_t)4 * iters);
    solver_coefficients(alphas_.data(), n_train_, n_steps, step_start, solver_, eta, c2m.data());
  }
  for (int i = 0; i < iters; ++i) {
    const int t = ts[i];
    const double a = alphas_[t];
    const double ap = t >= step_size ? alphas_[t - step_size] : 1.0;
    StepCoef k{};
    k.t = (float)t;
    k.sqrt_a = (float)std::sqrt(a);
    k.sqrt_1ma = (float)std::sqrt(1.0 - a);
    k.cfg = (float)cfg_scale;
    if (solver_ == kSolverDpmpp2M) {
      k.c_x = (float)c2m[4 * i]; k.c_0 = (float)c2m[4 * i + 1]; k.c_1 = (float)c2m[4 * i + 2]; k.c_z = (float)c2m[4 * i + 3];
    } else {
      double sqrt_ap, sqrt_1map, sigma;
      ddim_terms(a, ap, eta, sqrt_ap, sqrt_1map, sigma);
      k.sqrt_ap = (float)sqrt_ap;
      k.sqrt_1map = (float)sqrt_1map;
      k.sigma = (float)sigma;
    }
    tab[i] = k;
    if (guided) act[i] = t >= go.t_lo && t <= go.t_hi;
  }
  tab[iters] = StepCoef{};
  if (iters + 1 > table_cap_) {
    if (table_) SDXL_HIP(hipFree(table_));
    SDXL_HIP(hipMalloc((void**)&table_, (size_t)(iters + 1) * sizeof(StepCoef)));
    table_cap_ = iters + 1;
  }
  SDXL_HIP(hipMemcpyAsync(table_, tab.data(), (size_t)(iters + 1) * sizeof(StepCoef), hipMemcpyHostToDevice, s));
  GuidedParams gp{};
  if (guided) {
    if (iters > active_cap_) {
      if (active_) SDXL_HIP(hipFree(active_));
      active_ = nullptr;
      SDXL_HIP(hipMalloc((void**)&active_, (size_t)iters * sizeof(int)));
      active_cap_ = iters;
    }
    SDXL_HIP(hipMemcpyAsync(active_, act.data(), (size_t)iters * sizeof(int), hipMemcpyHostToDevice, s));
    for (int b = 0; b < n; ++b) gp.scales.v[b] = go.n_scales ? go.scales[b] : (float)cfg_scale;
    gp.active = active_;
    if (go.rescale > 0.f) {
      ensure_latent(moments_, moments_cap_, cfg_moments_floats(n, HW));
      if (!factors_) SDXL_HIP(hipMalloc((void**)&factors_, kMaxSeeds * sizeof(float)));
      gp.factors = factors_;
    }
  }
  SDXL_HIP(hipStreamSynchronize(s));   // tab is a stack-owned host buffer

  DdimParams p{};
  p.latent = latent;
  p.eps = u.eps_out(); p.eps_dt = DT_F32; p.eps_ld = uc.out_channels;
  p.table = table_; p.step_idx = step_idx_;
  p.n = n; p.HW = HW; p.use_cfg = single ? 0 : 1;
  p.ref = reference; p.mask = mask; p.step_noise = step_noise; p.n_steps_total = iters;
  p.unet_in = unet_in; p.in_dt = u.input_dt(); p.in_ld = uc.in_channels; p.in_rep = single ? 1 : 2;
  p.t_out = t_dev_;
  p.solver = solver_; p.hist = hist_;
  if (seeds) {
    p.seeded = 1;
    for (int b = 0; b < n; ++b) p.seeds.v[b] = seeds[b];
  }
  launch_ddim_step(p, 0, s);

  std::vector<hipEvent_t> ev;
  if (time_steps) {
    ev.resize(iters + 1);
    for (auto& e : ev) SDXL_HIP(hipEventCreate(&e));
    SDXL_HIP(hipEventRecord(ev[0], s));
  }
  for (int i = 0; i < iters; ++i) {
    u.forward(B, h, w, t_dev_, 0, s);     // one timestep shared by every batch entry (:416)
    if (guided) {     // moments, factor, step on an active iteration with rescale; the step kernel alone otherwise
      if (gp.factors && act[i]) launch_cfg_rescale_factors(p.eps, p.eps_dt, p.eps_ld, n, HW, gp.scales, go.rescale, moments_, factors_, s);
      launch_guided_step(p, gp, s);
    } else {
      launch_ddim_step(p, 1, s);
    }
    if (trace && i < trace_cap)
      SDXL_HIP(hipMemcpyAsync(trace + (size_t)i * n * 4 * HW, latent, (size_t)n * 4 * HW * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (time_steps) SDXL_HIP(hipEventRecord(ev[i + 1], s));
  }
  if (time_steps) {
    SDXL_HIP(hipEventSynchronize(ev[iters]));
    step_ms.assign(iters, 0.f);
    for (int i = 0; i < iters; ++i) SDXL_HIP(hipEventElapsedTime(&step_ms[i], ev[i], ev[i + 1]));
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
}

void Diffuser::ensure_state(size_t elems) {
  ensure_latent(latent_, latent_cap_, elems);
  if (solver_ == kSolverDpmpp2M) ensure_latent(hist_, hist_cap_, elems);
}

void Diffuser::sample_latent(const Conditioning& c, double cfg_scale, int n_steps, const float* noise0, float* out,
                             hipStream_t s) {
  const size_t elems = (size_t)c.n * 4 * (c.height / 8) * (c.width / 8);
  ensure_state(elems);
  SDXL_HIP(hipMemcpyAsync(latent_, noise0, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
  diffuse(latent_, c, 0, n_steps, cfg_scale, nullptr, nullptr, nullptr, s);
  SDXL_HIP(hipMemcpyAsync(out, latent_, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void Diffuser::sample_latent_inpaint(const Conditioning& c, double cfg_scale, int n_steps, const float* reference,
                                     const unsigned char* mask, const float* noise0, const float* step_noise, float* out,
                                     hipStream_t s) {
  SDXL_REQUIRE(reference && mask && step_noise, "inpainting needs reference, mask and per-step noise");
  const size_t elems = (size_t)c.n * 4 * (c.height / 8) * (c.width / 8);
  ensure_state(elems);
  SDXL_HIP(hipMemcpyAsync(latent_, noise0, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
  diffuse(latent_, c, 0, n_steps, cfg_scale, reference, mask, step_noise, s);
  SDXL_HIP(hipMemcpyAsync(out, latent_, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void Diffuser::refine_latent(const float* latent, const Conditioning& c, double cfg_scale, int step_start, int n_steps,
                             const float* noise, float* out, hipStream_t s) {
  // :355-376: re-noise the finished latent to t = n_train - step_start, then denoise from there
  SDXL_REQUIRE(step_start >= 1 && step_start <= n_train_, "step_start out of range");
  const size_t elems = (size_t)c.n * 4 * (c.height / 8) * (c.width / 8);
  ensure_state(elems);
  const double a = alphas_[n_train_ - step_start];
  launch_axpby(latent_, latent, (float)std::sqrt(a), noise, (float)std::sqrt(1.0 - a), elems, s);
  diffuse(latent_, c, step_start, n_steps, cfg_scale, nullptr, nullptr, nullptr, s);
  SDXL_HIP(hipMemcpyAsync(out, latent_, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
}

// The seeded forms: same trajectories, noise from launch_seeded_noise / the seeded per-step kernel.
void Diffuser::sample_latent_seeded(const Conditioning& c, double cfg_scale, int n_steps, const uint64_t* seeds, double eta,
                                    float* out, hipStream_t s) {
  SDXL_REQUIRE(c.n <= kMaxSeeds, "batch out of range");
  const int HW = (c.height / 8) * (c.width / 8);
  const size_t elems = (size_t)c.n * 4 * HW;
  ensure_state(elems);
  launch_seeded_noise(latent_, seeds, kDrawInitial, c.n, HW, s);
  diffuse(latent_, c, 0, n_steps, cfg_scale, nullptr, nullptr, nullptr, s, seeds, eta);
  SDXL_HIP(hipMemcpyAsync(out, latent_, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void Diffuser::sample_latent_inpaint_seeded(const Conditioning& c, double cfg_scale, int n_steps, const float* reference,
                                            const unsigned char* mask, const uint64_t* seeds, double eta, float* out,
                                            hipStream_t s) {
  SDXL_REQUIRE(reference && mask, "inpainting needs reference and mask");
  SDXL_REQUIRE(c.n <= kMaxSeeds, "batch out of range");
  const int HW = (c.height / 8) * (c.width / 8);
  const size_t elems = (size_t)c.n * 4 * HW;
  ensure_state(elems);
  launch_seeded_noise(latent_, seeds, kDrawInitial, c.n, HW, s);
  diffuse(latent_, c, 0, n_steps, cfg_scale, reference, mask, nullptr, s, seeds, eta);
  SDXL_HIP(hipMemcpyAsync(out, latent_, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void Diffuser::refine_latent_seeded(const float* latent, const Conditioning& c, double cfg_scale, int step_start, int n_steps,
                                    const uint64_t* seeds, double eta, float* out, hipStream_t s) {
  SDXL_REQUIRE(step_start >= 1 && step_start <= n_train_, "step_start out of range");
  SDXL_REQUIRE(c.n <= kMaxSeeds, "batch out of range");
  const int HW = (c.height / 8) * (c.width / 8);
  const size_t elems = (size_t)c.n * 4 * HW;
  ensure_state(elems);
  ensure_latent(noise_, noise_cap_, elems);
  launch_seeded_noise(noise_, seeds, kDrawInitial, c.n, HW, s);
  const double a = alphas_[n_train_ - step_start];
  launch_axpby(latent_, latent, (float)std::sqrt(a), noise_, (float)std::sqrt(1.0 - a), elems, s);
  diffuse(latent_, c, step_start, n_steps, cfg_scale, nullptr, nullptr, nullptr, s, seeds, eta);
  SDXL_HIP(hipMemcpyAsync(out, latent_, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
}

}  // namespace sdxl
