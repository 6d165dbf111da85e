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
//     batch-n forward; or per-entry scales, a timestep interval and CFG rescale -- arguments of the same per-step kernel, with two small launches
//     in front of it where rescale is on.  The default options are the call's scalar as every entry's scale.
//   * what the UNet's output means is a per-handle choice as well (set_prediction): the noise e, or v = alpha e - sigma x0, in further instantiations
//     of the same kernel (x0 = alpha x - sigma v, no division).  With v a schedule may hold alphas_cumprod == 0 at an iteration's timestep (zero
//     terminal SNR); the table's row there is written as the limit lambda -> -inf, and under e such a schedule is refused before anything is launched.
//   * which timesteps a trajectory visits is a per-handle choice (set_timesteps): the reference's rule by default, or any strictly decreasing list.
//     The list is the only source of an iteration's (t, a, ap) -- ap is the alpha of the next entry, 1 behind the last -- for the table, the guidance
//     interval, the trace and the t fed to the UNet.  On it run DDIM and 2M as before and the consistency solvers of distilled checkpoints (LCM, TCD):
//     first-order rows of the same table that re-noise with the seeded z every iteration, in one more instantiation of the same kernel.
// StepLoop is everything between two UNet forwards; Diffuser::diffuse is context setup and the loop around UNet::forward.
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
}
Diffuser::~Diffuser() {
  for (void* p : {(void*)latent_, (void*)noise_, (void*)ctx_buf_, (void*)y_buf_})
    if (p) (void)hipFree(p);
}

// sigma (:423 pins it to 0.0): standard DDIM eta; ap = 1 on the last iteration, so nothing is drawn there
static void ddim_terms(double a, double ap, double eta, double& sqrt_ap, double& sqrt_1map, double& sigma) {
  sigma = eta == 0.0 ? 0.0 : eta * std::sqrt((1.0 - ap) / (1.0 - a)) * std::sqrt(1.0 - a / ap);
  sqrt_ap = std::sqrt(ap);
  sqrt_1map = std::sqrt(std::max(1.0 - ap - sigma * sigma, 0.0));
}

void Diffuser::set_solver(int solver) {
  SDXL_REQUIRE(solver == kSolverDdim || solver == kSolverDpmpp2M || solver_is_row1(solver), "unknown solver");
  solver_ = solver;
}

const char* Diffuser::timesteps_error(const int* ts, int n, int n_train) {
  if (!ts || n < 1 || n > n_train) return "timesteps: the list needs 1..n_train_steps entries";
  for (int i = 0; i < n; ++i) {
    if (ts[i] < 0 || ts[i] >= n_train) return "timesteps: a value outside 0..n_train_steps-1";
    if (i > 0 && ts[i] >= ts[i - 1]) return "timesteps: the list must be strictly decreasing";
  }
  return nullptr;
}
void Diffuser::set_timesteps(const int* ts, int n) {
  if (!ts || n == 0) { timesteps_.clear(); return; }
  if (const char* m = timesteps_error(ts, n, n_train_)) throw InvalidArgumentError(m);
  timesteps_.assign(ts, ts + n);
}

std::vector<int> Diffuser::call_schedule(int n_steps, int step_start, bool renoise) const {
  if (timesteps_.empty()) return step_schedule(n_steps, step_start, n_train_);
  if (n_steps != (int)timesteps_.size())
    throw InvalidArgumentError("timesteps: n_steps (" + std::to_string(n_steps) + ") differs from the length of the handle's list (" +
                               std::to_string(timesteps_.size()) + ")");
  if (!renoise && step_start != 0) throw InvalidArgumentError("timesteps: step_start must be 0 where a list is set");
  if (renoise && timesteps_[0] != n_train_ - step_start - 1)
    throw InvalidArgumentError("timesteps: refine_latent re-noises to n_train_steps - step_start, so the list must start at n_train_steps - step_start - 1");
  return timesteps_;
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

const char* control_error(const Control& c, bool single) {
  if (!std::isfinite(c.scale)) return "control: scale must be finite";
  if (c.n_scales < 0 || c.n_scales > kMaxSeeds) return "control: n_scales out of range (0..8)";
  for (int b = 0; b < c.n_scales; ++b)
    if (!std::isfinite(c.scales[b])) return "control: scales must be finite";
  if (c.t_lo < 0 || c.t_lo > c.t_hi) return "control: interval needs 0 <= t_lo <= t_hi";
  if (c.cond_only && single) return "control: cond_only needs the CFG pair; a single branch (SDXL_GUIDANCE_OFF) has no unconditional entries";
  return nullptr;
}

const char* control_scale_table(const Control& c, int n, bool single, const int* timesteps, int iters, float* out) {
  if (const char* m = control_error(c, single)) return m;
  if (n < 1 || (single ? n : 2 * n) > kMaxSeeds) return "control: batch out of range (n in 1..8, 1..4 with the CFG pair)";
  if (c.n_scales != 0 && c.n_scales != n) return "control: n_scales differs from the batch (cond.n)";
  if (iters < 0 || (iters > 0 && !timesteps) || !out) return "control: null argument";
  const int B = single ? n : 2 * n;
  for (int i = 0; i <= iters; ++i) {
    float* row = out + (size_t)i * kMaxSeeds;
    const bool on = i < iters && timesteps[i] >= c.t_lo && timesteps[i] <= c.t_hi;      // row `iters`: the sentinel a step index rests on
    for (int b = 0; b < kMaxSeeds; ++b)
      row[b] = on && b < B && !(c.cond_only && b >= n) ? (c.n_scales ? c.scales[b % n] : c.scale) : 0.f;
  }
  return nullptr;
}

void Diffuser::set_prediction(int prediction) {
  SDXL_REQUIRE(prediction == kPredictionEpsilon || prediction == kPredictionV, "unknown prediction");
  prediction_ = prediction;
}

const char* Diffuser::schedule_error(const double* alphas, int n_train, const std::vector<int>& ts, int prediction) {
  if (prediction != kPredictionEpsilon && prediction != kPredictionV) return "unknown prediction (SDXL_PREDICTION_EPSILON, SDXL_PREDICTION_V)";
  if (!ts.empty())             // (refine_latent at step_start == n_train: no iteration, nothing to complain about)
    if (const char* m = timesteps_error(ts.data(), (int)ts.size(), n_train)) return m;
  for (size_t i = 0; i < ts.size(); ++i) {
    const double a = alphas[ts[i]];
    const double ap = i + 1 < ts.size() ? alphas[ts[i + 1]] : 1.0;
    if (prediction == kPredictionEpsilon) {
      if (a == 0.0)
        return "alphas_cumprod is 0 at a sampled timestep (zero terminal SNR): x0 = (x - sigma e) / alpha has no value there under the "
               "epsilon prediction; such a schedule needs v-prediction (SDXL_PREDICTION_V)";
    } else if (!(a >= 0.0 && a < 1.0 && ap > 0.0 && ap <= 1.0)) {
      return "prediction v: alphas_cumprod outside [0, 1) at a sampled timestep, or 0 at the timestep a step lands on";
    }
  }
  return nullptr;
}

void Diffuser::solver_coefficients(const double* alphas, int n_train, const std::vector<int>& ts, int solver, double eta, double* out,
                                   int prediction) {
  SDXL_REQUIRE(solver == kSolverDdim || solver == kSolverDpmpp2M || solver_is_row1(solver), "unknown solver");
  if (const char* m = schedule_error(alphas, n_train, ts, prediction)) throw InvalidArgumentError(m);
  if (solver == kSolverLcm && eta != 0.0) throw InvalidArgumentError("solver LCM takes no eta: eta must be 0 (SDXL_SOLVER_LCM)");
  double h_prev = 0.0;
  bool have_prev = false;       // false on iteration 0: no history, first order
  for (size_t i = 0; i < ts.size(); ++i) {
    const int t = ts[i];
    const double a = alphas[t];
    const double ap = i + 1 < ts.size() ? alphas[ts[i + 1]] : 1.0;      // the next entry of the list; behind the last one the data itself
    SDXL_REQUIRE((a > 0.0 || (a == 0.0 && prediction == kPredictionV)) && a < 1.0 && ap > 0.0 && ap <= 1.0, "alphas_cumprod outside (0, 1)");
    const double alpha = std::sqrt(a), sigma = std::sqrt(1.0 - a);
    double* c = out + 4 * i;     // c_x, c_0, c_1, c_z
    if (solver == kSolverDdim) {
      double sqrt_ap, sqrt_1map, sigma_t;
      ddim_terms(a, ap, eta, sqrt_ap, sqrt_1map, sigma_t);
      c[0] = sqrt_1map / sigma; c[1] = sqrt_ap - sqrt_1map * alpha / sigma; c[2] = 0.0; c[3] = sigma_t;
      continue;
    }
    if (solver == kSolverLcm) {  // diffusers' LCMScheduler.step: sigma_data = 0.5, timestep_scaling = 10; the boundary-condition pair of x0, then
                                 // re-noised to the next level with fresh noise.  ap == 1 behind the last entry: (c_skip, c_out, 0, 0)
      const double st = 10.0 * (double)t, d = st * st + 0.25;
      const double c_skip = 0.25 / d, c_out = st / std::sqrt(d);
      const double alpha_p = std::sqrt(ap);
      c[0] = alpha_p * c_skip; c[1] = alpha_p * c_out; c[2] = 0.0; c[3] = std::sqrt(1.0 - ap);
      continue;
    }
    if (solver == kSolverTcd) {  // TCDScheduler.step, eta read as gamma: the DDIM step to s = floor((1 - gamma) t'), re-noised from s to t'
      if (ap == 1.0) {           // the engine's last row, as 2M has it: the iteration returns x0
        c[0] = 0.0; c[1] = 1.0; c[2] = 0.0; c[3] = 0.0;
        continue;
      }
      const int ts_s = (int)std::floor((1.0 - eta) * (double)ts[i + 1]);
      const double a_s = alphas[ts_s];
      if (!(a_s > 0.0 && a_s <= 1.0)) throw InvalidArgumentError("solver TCD: alphas_cumprod outside (0, 1] at the timestep floor((1 - gamma) t')");
      const double alpha_s = std::sqrt(a_s), sigma_s = std::sqrt(1.0 - a_s), r = std::sqrt(ap / a_s);
      c[0] = r * sigma_s / sigma; c[1] = r * (alpha_s - sigma_s * alpha / sigma); c[2] = 0.0;
      c[3] = std::sqrt(std::max(1.0 - ap / a_s, 0.0));
      continue;
    }
    if (ap == 1.0) {             // h is infinite: the step lands on the data prediction
      c[0] = 0.0; c[1] = 1.0; c[2] = 0.0; c[3] = 0.0;
      have_prev = false;
      continue;
    }
    const double alpha_p = std::sqrt(ap), sigma_p = std::sqrt(1.0 - ap);
    if (a == 0.0) {              // alpha = 0, sigma = 1, lambda = -inf, h = +inf: the limits of the first-order row, written out (the formulas
                                 // below would evaluate exp(-0 * inf)).  A -> 1; eta == 0: c_x = sigma'; eta > 0: c_x -> 0, c_z -> sigma'
      c[0] = eta == 0.0 ? sigma_p : 0.0; c[1] = alpha_p; c[2] = 0.0; c[3] = eta == 0.0 ? 0.0 : sigma_p;
      have_prev = false;         // the next iteration has r = h_prev / h = inf: first order, as iteration 0
      continue;
    }
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

const char* Diffuser::explicit_noise_error(const double* alphas, int n_train, const std::vector<int>& ts, int solver, int prediction) {
  if (!solver_is_row1(solver)) return nullptr;      // DDIM and 2M at eta == 0 draw nothing
  std::vector<double> rows((size_t)4 * ts.size());
  solver_coefficients(alphas, n_train, ts, solver, 0.0, rows.data(), prediction);
  for (size_t i = 0; i < ts.size(); ++i)
    if (rows[4 * i + 3] != 0.0)
      return "this solver re-noises with fresh noise every iteration (c_z != 0): it needs the seeded calls (explicit noise carries none for that term)";
  return nullptr;
}

#ifdef SDXL_MEASURE
bool g_debug_no_cfg = false;
#else
static constexpr bool g_debug_no_cfg = false;
#endif

template <class T, class N>
static void ensure_device(T*& buf, N& cap, size_t elems) {     // a device buffer of at least `elems` values; grows, never shrinks
  if (elems > (size_t)cap) {
    if (buf) SDXL_HIP(hipFree(buf));
    buf = nullptr;
    SDXL_HIP(hipMalloc((void**)&buf, elems * sizeof(T)));
    cap = (N)elems;
  }
}

// ------------------------------------------------------------------------------------------ StepLoop
StepLoop::StepLoop() {
  SDXL_HIP(hipMalloc((void**)&step_idx_, sizeof(int)));
  SDXL_HIP(hipMalloc((void**)&t_dev_, 8 * sizeof(float)));
}
StepLoop::~StepLoop() {
  for (void* p : {(void*)table_, (void*)active_, (void*)moments_, (void*)factors_, (void*)step_idx_, (void*)t_dev_, (void*)hist_})
    if (p) (void)hipFree(p);
}

int StepLoop::begin(const std::vector<double>& alphas, const std::vector<int>& ts, int solver, double eta, double cfg_scale,
                    const Guidance& go, bool single, int n, int HW, const StepIo& io, hipStream_t s, int prediction) {
  const int n_train = (int)alphas.size();
  SDXL_REQUIRE(n >= 1 && n <= kMaxSeeds, "batch out of range");
  // a == 0 on an iteration: x0 = -v under kPredictionV; under kPredictionEpsilon the first update would divide by sqrt_a == 0
  if (const char* m = Diffuser::schedule_error(alphas.data(), n_train, ts, prediction)) throw InvalidArgumentError(m);
  SDXL_REQUIRE(single || go.n_scales == 0 || go.n_scales == n, "guidance: n_scales differs from the batch (cond.n)");
  const bool rows = solver != kSolverDdim;             // the 2M layout of the table: 2M itself and the first-order rows of LCM / TCD
  if (!io.seeds)
    if (const char* m = Diffuser::explicit_noise_error(alphas.data(), n_train, ts, solver, prediction)) throw InvalidArgumentError(m);
  // --- coefficient table (host f64, exactly the reference's scalar arithmetic :407-414, :423-426)
  const int iters = (int)ts.size();
  std::vector<StepCoef> tab(iters + 1);
  act_.assign(iters, 1);                               // guidance interval: iteration i is active where t_lo <= t_i <= t_hi
  std::vector<double> c2m;
  if (rows) {
    c2m.resize((size_t)4 * iters);
    Diffuser::solver_coefficients(alphas.data(), n_train, ts, solver, eta, c2m.data(), prediction);
  }
  for (int i = 0; i < iters; ++i) {
    const int t = ts[i];
    const double a = alphas[t];
    const double ap = i + 1 < iters ? alphas[ts[i + 1]] : 1.0;
    StepCoef k{};
    k.t = (float)t;
    k.sqrt_a = (float)std::sqrt(a);
    k.sqrt_1ma = (float)std::sqrt(1.0 - a);
    if (rows) {
      k.c_x = (float)c2m[4 * i]; k.c_0 = (float)c2m[4 * i + 1]; k.c_1 = (float)c2m[4 * i + 2]; k.c_z = (float)c2m[4 * i + 3];
    } else {
      double sqrt_ap, sqrt_1map, sigma;
      ddim_terms(a, ap, eta, sqrt_ap, sqrt_1map, sigma);
      k.sqrt_ap = (float)sqrt_ap;
      k.sqrt_1map = (float)sqrt_1map;
      k.sigma = (float)sigma;
    }
    tab[i] = k;
    if (!single) act_[i] = t >= go.t_lo && t <= go.t_hi;
  }
  tab[iters] = StepCoef{};
  ensure_device(table_, table_cap_, (size_t)iters + 1);
  SDXL_HIP(hipMemcpyAsync(table_, tab.data(), (size_t)(iters + 1) * sizeof(StepCoef), hipMemcpyHostToDevice, s));
  p_ = StepParams{};
  rescale_ = single ? 0.f : go.rescale;
  // the default options are the call's scalar for every entry -- the float the kernel always multiplied by -- no interval array, no factors
  for (int b = 0; b < n; ++b) p_.scales.v[b] = !single && go.n_scales ? go.scales[b] : (float)cfg_scale;
  if (std::find(act_.begin(), act_.end(), 0) != act_.end()) {
    ensure_device(active_, active_cap_, (size_t)iters);
    SDXL_HIP(hipMemcpyAsync(active_, act_.data(), (size_t)iters * sizeof(int), hipMemcpyHostToDevice, s));
    p_.active = active_;
  }
  if (rescale_ > 0.f) {
    ensure_device(moments_, moments_cap_, cfg_moments_floats(n, HW));
    if (!factors_) SDXL_HIP(hipMalloc((void**)&factors_, kMaxSeeds * sizeof(float)));
    p_.factors = factors_;
  }
  if (solver == kSolverDpmpp2M) ensure_device(hist_, hist_cap_, (size_t)n * 4 * HW);      // kSolverRow1 keeps no history: nothing is allocated
  SDXL_HIP(hipStreamSynchronize(s));   // tab is a stack-owned host buffer

  p_.latent = io.latent;
  p_.eps_dt = DT_F32; p_.eps_ld = io.eps_ld;
  p_.table = table_; p_.step_idx = step_idx_;
  p_.n = n; p_.HW = HW; p_.use_cfg = single ? 0 : 1;
  p_.ref = io.reference; p_.mask = io.mask; p_.step_noise = io.step_noise; p_.n_steps_total = iters;
  p_.unet_in = io.unet_in; p_.in_dt = io.in_dt; p_.in_ld = io.in_ld; p_.in_rep = single ? 1 : 2;
  p_.t_out = t_dev_;
  p_.solver = solver_is_row1(solver) ? kSolverRow1 : solver; p_.prediction = prediction;
  p_.hist = solver_is_row1(solver) ? nullptr : hist_;
  if (io.seeds) {
    p_.seeded = 1;
    for (int b = 0; b < n; ++b) p_.seeds.v[b] = io.seeds[b];
  }
  launch_step(p_, 0, s);
  return iters;
}

void StepLoop::after_forward(int i, const float* eps, hipStream_t s) {
  p_.eps = eps;
  // CFG rescale: moments and factor in front of the step on an active iteration
  if (p_.factors && act_[i]) launch_cfg_rescale_factors(eps, p_.eps_dt, p_.eps_ld, p_.n, p_.HW, p_.scales, rescale_, moments_, factors_, s);
  launch_step(p_, 1, s);
}

// ------------------------------------------------------------------------------------------ Diffuser
void Diffuser::diffuse(float* latent, const Conditioning& c, const std::vector<int>& ts, double cfg_scale,
                       const float* reference, const unsigned char* mask, const float* step_noise, hipStream_t s,
                       const uint64_t* seeds, double eta) {
  // diffuse_latent :390-432 / diffuse_latent_with_inpainting :434-483
  UNet& u = *unet_;
  const UNetCfg& uc = u.cfg();
  const Guidance& go = guidance_;
  // kGuidanceOff: conditional branch only, as for a refiner (debug knob: the same for concurrency experiments)
  const bool single = is_refiner_ || go.mode == kGuidanceOff || g_debug_no_cfg;
  const int n = c.n, B = single ? n : 2 * n;
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
  ensure_device(ctx_buf_, ctx_cap_, (size_t)B * ctx_elems);
  ensure_device(y_buf_, y_cap_, (size_t)B * adm);
  SDXL_HIP(hipMemcpyAsync(ctx_buf_, ctx, (size_t)n * ctx_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
  SDXL_HIP(hipMemcpyAsync(y_buf_, y, (size_t)n * adm * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (!single)
    for (int i = 0; i < n; ++i) {   // unconditional_context.unsqueeze().repeat(0, n_batch) :535-536
      SDXL_HIP(hipMemcpyAsync(ctx_buf_ + (size_t)(n + i) * ctx_elems, uctx, ctx_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
      SDXL_HIP(hipMemcpyAsync(y_buf_ + (size_t)(n + i) * adm, uy, adm * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  StepIo io{};
  io.latent = latent; io.eps_ld = uc.out_channels;
  io.unet_in = u.unet_in(B, h, w); io.in_dt = u.input_dt(); io.in_ld = uc.in_channels;
  io.reference = reference; io.mask = mask; io.step_noise = step_noise; io.seeds = seeds;
  u.set_context(ctx_buf_, c.n_ctx, y_buf_, B, s);

  const int iters = loop_.begin(alphas_, ts, solver_, eta, cfg_scale, go, single, n, HW, io, s, prediction_);
  std::vector<hipEvent_t> ev;
  if (time_steps) {
    ev.resize(iters + 1);
    for (auto& e : ev) SDXL_HIP(hipEventCreate(&e));
    SDXL_HIP(hipEventRecord(ev[0], s));
  }
  for (int i = 0; i < iters; ++i) {
    u.forward(B, h, w, loop_.t_dev(), 0, s);     // one timestep shared by every batch entry (:416)
    loop_.after_forward(i, (const float*)u.eps_out(), s);
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

// Prologue and epilogue of the six trajectory calls.  The trajectory starts from t.noise (seeds: the kDrawInitial tensor of the entries' seeds)
// or, where t.renoise is given, from that latent re-noised to t = n_train - step_start (:355-376); then diffuse and the copy out.
void Diffuser::trajectory(const Conditioning& c, double cfg_scale, int n_steps, const Trajectory& t, float* out, hipStream_t s) {
  SDXL_REQUIRE(!t.renoise || (t.step_start >= 1 && t.step_start <= n_train_), "step_start out of range");
  SDXL_REQUIRE(!t.seeds || c.n <= kMaxSeeds, "batch out of range");
  // what StepLoop::begin refuses, before the start latent is written: nothing is launched
  const std::vector<int> ts = call_schedule(n_steps, t.step_start, t.renoise != nullptr);
  if (const char* m = schedule_error(alphas_.data(), n_train_, ts, prediction_)) throw InvalidArgumentError(m);
  if (solver_ == kSolverLcm && t.eta != 0.0) throw InvalidArgumentError("solver LCM takes no eta: eta must be 0 (SDXL_SOLVER_LCM)");
  if (!t.seeds)
    if (const char* m = explicit_noise_error(alphas_.data(), n_train_, ts, solver_, prediction_)) throw InvalidArgumentError(m);
  const int HW = (c.height / 8) * (c.width / 8);
  const size_t elems = (size_t)c.n * 4 * HW;
  ensure_device(latent_, latent_cap_, elems);
  if (t.renoise) {
    const float* noise = t.noise;
    if (t.seeds) {
      ensure_device(noise_, noise_cap_, elems);
      launch_seeded_noise(noise_, t.seeds, kDrawInitial, c.n, HW, s);
      noise = noise_;
    }
    const double a = alphas_[n_train_ - t.step_start];
    launch_axpby(latent_, t.renoise, (float)std::sqrt(a), noise, (float)std::sqrt(1.0 - a), elems, s);
  } else if (t.seeds) {
    launch_seeded_noise(latent_, t.seeds, kDrawInitial, c.n, HW, s);
  } else {
    SDXL_HIP(hipMemcpyAsync(latent_, t.noise, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  diffuse(latent_, c, ts, cfg_scale, t.reference, t.mask, t.step_noise, s, t.seeds, t.eta);
  SDXL_HIP(hipMemcpyAsync(out, latent_, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void Diffuser::sample_latent(const Conditioning& c, double cfg_scale, int n_steps, const float* noise0, float* out,
                             hipStream_t s) {
  Trajectory t; t.noise = noise0;
  trajectory(c, cfg_scale, n_steps, t, out, s);
}

void Diffuser::sample_latent_inpaint(const Conditioning& c, double cfg_scale, int n_steps, const float* reference,
                                     const unsigned char* mask, const float* noise0, const float* step_noise, float* out,
                                     hipStream_t s) {
  SDXL_REQUIRE(reference && mask && step_noise, "inpainting needs reference, mask and per-step noise");
  Trajectory t; t.noise = noise0; t.reference = reference; t.mask = mask; t.step_noise = step_noise;
  trajectory(c, cfg_scale, n_steps, t, out, s);
}

void Diffuser::refine_latent(const float* latent, const Conditioning& c, double cfg_scale, int step_start, int n_steps,
                             const float* noise, float* out, hipStream_t s) {
  Trajectory t; t.renoise = latent; t.step_start = step_start; t.noise = noise;
  trajectory(c, cfg_scale, n_steps, t, out, s);
}

// The seeded forms: same trajectories, noise from launch_seeded_noise / the seeded per-step kernel.
void Diffuser::sample_latent_seeded(const Conditioning& c, double cfg_scale, int n_steps, const uint64_t* seeds, double eta,
                                    float* out, hipStream_t s) {
  Trajectory t; t.seeds = seeds; t.eta = eta;
  trajectory(c, cfg_scale, n_steps, t, out, s);
}

void Diffuser::sample_latent_inpaint_seeded(const Conditioning& c, double cfg_scale, int n_steps, const float* reference,
                                            const unsigned char* mask, const uint64_t* seeds, double eta, float* out,
                                            hipStream_t s) {
  SDXL_REQUIRE(reference && mask, "inpainting needs reference and mask");
  Trajectory t; t.seeds = seeds; t.eta = eta; t.reference = reference; t.mask = mask;
  trajectory(c, cfg_scale, n_steps, t, out, s);
}

void Diffuser::refine_latent_seeded(const float* latent, const Conditioning& c, double cfg_scale, int step_start, int n_steps,
                                    const uint64_t* seeds, double eta, float* out, hipStream_t s) {
  Trajectory t; t.renoise = latent; t.step_start = step_start; t.seeds = seeds; t.eta = eta;
  trajectory(c, cfg_scale, n_steps, t, out, s);
}

}  // namespace sdxl
