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
//   * the list itself is a Schedule of noise levels: (t, a) per iteration and the level behind the last one.  An integer list fills it
//     from the table; a sigma list (Karras, exponential, hand-tuned) with a = 1 / (1 + sigma^2) and a fractional t; an end level other than the data
//     stops a trajectory early, and continue_latent starts one from a given latent: the base -> refiner handoff without re-noising.  DPM++ 3M SDE is
//     the 2M row with a second history term, in four more instantiations of the same kernel.
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
  SDXL_REQUIRE(solver == kSolverDdim || solver == kSolverDpmpp2M || solver == kSolverDpmpp3M || solver_is_row1(solver), "unknown solver");
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
const char* Diffuser::timesteps_end_error(const int* ts, int n, int t_end, int n_train) {
  if (const char* m = timesteps_error(ts, n, n_train)) return m;
  if (t_end < -1 || t_end >= ts[n - 1]) return "timesteps: t_end must lie below the last entry (-1: the complete trajectory)";
  return nullptr;
}
void Diffuser::set_timesteps(const int* ts, int n, int t_end) {
  if (!ts || n == 0) { timesteps_.clear(); timesteps_end_ = -1; sigmas_.clear(); return; }
  if (const char* m = timesteps_end_error(ts, n, t_end, n_train_)) throw InvalidArgumentError(m);
  timesteps_.assign(ts, ts + n);
  timesteps_end_ = t_end;
  sigmas_.clear();
}

const char* Diffuser::sigmas_error(const double* sigmas, int n, double sigma_end, int flags, int n_train) {
  if (n_train < 2) return "sigmas: the alphas_cumprod table needs at least two entries";
  if (!sigmas || n < 1 || n > n_train) return "sigmas: the list needs 1..n_train_steps entries";
  if ((flags & ~kSigmasRoundT) != 0) return "sigmas: unknown flags (SDXL_SIGMAS_ROUND_T)";
  for (int i = 0; i < n; ++i) {
    if (!(std::isfinite(sigmas[i]) && sigmas[i] > 0.0)) return "sigmas: a value that is not finite and > 0";
    if (i > 0 && !(sigmas[i] < sigmas[i - 1])) return "sigmas: the list must be strictly decreasing";
  }
  if (!(sigma_end >= 0.0 && sigma_end < sigmas[n - 1])) return "sigmas: sigma_end must lie in [0, the last entry) (0: the complete trajectory)";
  return nullptr;
}
void Diffuser::set_sigmas(const double* sigmas, int n, double sigma_end, int flags) {
  if (!sigmas || n == 0) { sigmas_.clear(); return; }
  if (const char* m = sigmas_error(sigmas, n, sigma_end, flags, n_train_)) throw InvalidArgumentError(m);
  sigmas_.assign(sigmas, sigmas + n);
  sigma_end_ = sigma_end;
  sigma_flags_ = flags;
}

double Diffuser::sigma_to_t(const double* alphas, int n_train, double sigma, int flags) {
  SDXL_REQUIRE(n_train >= 2, "sigmas: the alphas_cumprod table needs at least two entries");
  const auto L = [&](int j) { return 0.5 * std::log((1.0 - alphas[j]) / alphas[j]); };
  const double ls = std::log(sigma);
  int low = 0;
  for (int j = n_train - 2; j >= 0; --j)
    if (L(j) <= ls) { low = j; break; }
  const int high = low + 1;
  const double Ll = L(low), Lh = L(high);
  double w = (Ll - ls) / (Ll - Lh);
  w = !(w > 0.0) ? 0.0 : w > 1.0 ? 1.0 : w;      // clamp; a NaN (a table with equal neighbours) counts as 0
  const double t = (1.0 - w) * (double)low + w * (double)high;
  return (flags & kSigmasRoundT) ? std::nearbyint(t) : t;     // ties to even in the default rounding mode
}

Schedule Diffuser::schedule_of_timesteps(const double* alphas, int n_train, const int* ts, int n, int t_end) {
  Schedule sc;
  if (n == 0) return sc;        // (refine_latent at step_start == n_train: no iteration)
  if (const char* m = timesteps_end_error(ts, n, t_end, n_train)) throw InvalidArgumentError(m);
  sc.t.resize(n); sc.a.resize(n);
  for (int i = 0; i < n; ++i) { sc.t[i] = (double)ts[i]; sc.a[i] = alphas[ts[i]]; }
  sc.t_end = t_end;
  sc.a_end = t_end < 0 ? 1.0 : alphas[t_end];
  return sc;
}
Schedule Diffuser::schedule_of_sigmas(const double* alphas, int n_train, const double* sigmas, int n, double sigma_end, int flags) {
  if (const char* m = sigmas_error(sigmas, n, sigma_end, flags, n_train)) throw InvalidArgumentError(m);
  Schedule sc;
  sc.from_sigmas = true;
  sc.t.resize(n); sc.a.resize(n);
  for (int i = 0; i < n; ++i) {
    sc.a[i] = 1.0 / (1.0 + sigmas[i] * sigmas[i]);
    sc.t[i] = sigma_to_t(alphas, n_train, sigmas[i], flags);
  }
  sc.a_end = sigma_end == 0.0 ? 1.0 : 1.0 / (1.0 + sigma_end * sigma_end);
  return sc;
}

Schedule Diffuser::call_schedule(int n_steps, int step_start, bool renoise, bool listed_only) const {
  if (!sigmas_.empty()) {
    if (renoise)
      throw InvalidArgumentError("sigmas: refine_latent ties its re-noise level to step_start, which a sigma list does not have; re-noise to the "
                                 "list's first level with sdxl_continue_latent");
    if (n_steps != (int)sigmas_.size())
      throw InvalidArgumentError("sigmas: n_steps (" + std::to_string(n_steps) + ") differs from the length of the handle's list (" +
                                 std::to_string(sigmas_.size()) + ")");
    if (step_start != 0) throw InvalidArgumentError("sigmas: step_start must be 0 where a list is set");
    return schedule_of_sigmas(alphas_.data(), n_train_, sigmas_.data(), (int)sigmas_.size(), sigma_end_, sigma_flags_);
  }
  if (timesteps_.empty()) {
    if (listed_only) throw InvalidArgumentError("continue_latent runs the handle's list: set one first (sdxl_diffuser_set_sigmas, sdxl_diffuser_set_timesteps)");
    const std::vector<int> ts = step_schedule(n_steps, step_start, n_train_);
    return schedule_of_timesteps(alphas_.data(), n_train_, ts.data(), (int)ts.size());
  }
  if (n_steps != (int)timesteps_.size())
    throw InvalidArgumentError("timesteps: n_steps (" + std::to_string(n_steps) + ") differs from the length of the handle's list (" +
                               std::to_string(timesteps_.size()) + ")");
  if (!renoise && step_start != 0) throw InvalidArgumentError("timesteps: step_start must be 0 where a list is set");
  if (renoise && timesteps_[0] != n_train_ - step_start - 1)
    throw InvalidArgumentError("timesteps: refine_latent re-noises to n_train_steps - step_start, so the list must start at n_train_steps - step_start - 1");
  return schedule_of_timesteps(alphas_.data(), n_train_, timesteps_.data(), (int)timesteps_.size(), timesteps_end_);
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

const char* Diffuser::schedule_error(const Schedule& sc, int prediction) {
  if (prediction != kPredictionEpsilon && prediction != kPredictionV) return "unknown prediction (SDXL_PREDICTION_EPSILON, SDXL_PREDICTION_V)";
  for (size_t i = 0; i < sc.size(); ++i) {
    const double a = sc.a[i];
    const double ap = sc.ap(i);
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

void Diffuser::solver_coefficients(const double* alphas, int n_train, const Schedule& sc, int solver, double eta, double* out, int prediction) {
  SDXL_REQUIRE(solver == kSolverDdim || solver == kSolverDpmpp2M || solver == kSolverDpmpp3M || solver_is_row1(solver), "unknown solver");
  if (const char* m = schedule_error(sc, prediction)) throw InvalidArgumentError(m);
  if (solver == kSolverLcm && eta != 0.0) throw InvalidArgumentError("solver LCM takes no eta: eta must be 0 (SDXL_SOLVER_LCM)");
  if (solver == kSolverTcd && sc.from_sigmas)
    throw InvalidArgumentError("solver TCD reads alphas_cumprod at floor((1 - gamma) t'), a training timestep: it does not run on sigmas (use a timestep list)");
  double h_prev = 0.0, h_prev2 = 0.0;
  int order = 0;                // history terms at hand: 0 on iteration 0 (first order), at most 1 under 2M and 2 under 3M
  for (size_t i = 0; i < sc.size(); ++i) {
    const double t = sc.t[i];
    const double a = sc.a[i];
    const double ap = sc.ap(i);      // the next entry of the list; behind the last one the end level (1: the data itself)
    SDXL_REQUIRE((a > 0.0 || (a == 0.0 && prediction == kPredictionV)) && a < 1.0 && ap > 0.0 && ap <= 1.0, "alphas_cumprod outside (0, 1)");
    const double alpha = std::sqrt(a), sigma = std::sqrt(1.0 - a);
    double* c = out + kRowCols * i;     // c_x, c_0, c_1, c_2, c_z
    c[3] = 0.0;
    if (solver == kSolverDdim) {
      double sqrt_ap, sqrt_1map, sigma_t;
      ddim_terms(a, ap, eta, sqrt_ap, sqrt_1map, sigma_t);
      c[0] = sqrt_1map / sigma; c[1] = sqrt_ap - sqrt_1map * alpha / sigma; c[2] = 0.0; c[4] = sigma_t;
      continue;
    }
    if (solver == kSolverLcm) {  // diffusers' LCMScheduler.step: sigma_data = 0.5, timestep_scaling = 10; the boundary-condition pair of x0, then
                                 // re-noised to the next level with fresh noise.  ap == 1 behind the last entry: (c_skip, c_out, 0, 0)
      const double st = 10.0 * t, d = st * st + 0.25;
      const double c_skip = 0.25 / d, c_out = st / std::sqrt(d);
      const double alpha_p = std::sqrt(ap);
      c[0] = alpha_p * c_skip; c[1] = alpha_p * c_out; c[2] = 0.0; c[4] = std::sqrt(1.0 - ap);
      continue;
    }
    if (solver == kSolverTcd) {  // TCDScheduler.step, eta read as gamma: the DDIM step to s = floor((1 - gamma) t'), re-noised from s to t'
      if (ap == 1.0) {           // the engine's last row, as 2M has it: the iteration returns x0
        c[0] = 0.0; c[1] = 1.0; c[2] = 0.0; c[4] = 0.0;
        continue;
      }
      const double t_next = i + 1 < sc.size() ? sc.t[i + 1] : (double)sc.t_end;
      const int ts_s = (int)std::floor((1.0 - eta) * t_next);
      SDXL_REQUIRE(ts_s >= 0 && ts_s < n_train, "solver TCD: floor((1 - gamma) t') outside the table");
      const double a_s = alphas[ts_s];
      if (!(a_s > 0.0 && a_s <= 1.0)) throw InvalidArgumentError("solver TCD: alphas_cumprod outside (0, 1] at the timestep floor((1 - gamma) t')");
      const double alpha_s = std::sqrt(a_s), sigma_s = std::sqrt(1.0 - a_s), r = std::sqrt(ap / a_s);
      c[0] = r * sigma_s / sigma; c[1] = r * (alpha_s - sigma_s * alpha / sigma); c[2] = 0.0;
      c[4] = std::sqrt(std::max(1.0 - ap / a_s, 0.0));
      continue;
    }
    if (ap == 1.0) {             // h is infinite: the step lands on the data prediction
      c[0] = 0.0; c[1] = 1.0; c[2] = 0.0; c[4] = 0.0;
      order = 0;
      continue;
    }
    const double alpha_p = std::sqrt(ap), sigma_p = std::sqrt(1.0 - ap);
    if (a == 0.0) {              // alpha = 0, sigma = 1, lambda = -inf, h = +inf: the limits of the first-order row, written out (the formulas
                                 // below would evaluate exp(-0 * inf)).  A -> 1; eta == 0: c_x = sigma'; eta > 0: c_x -> 0, c_z -> sigma'
      c[0] = eta == 0.0 ? sigma_p : 0.0; c[1] = alpha_p; c[2] = 0.0; c[4] = eta == 0.0 ? 0.0 : sigma_p;
      order = 0;                 // the next iteration has r = h_prev / h = inf: first order, as iteration 0
      continue;
    }
    const double h = std::log(alpha_p / sigma_p) - std::log(alpha / sigma);
    const double A = -std::expm1(-(1.0 + eta) * h);
    c[0] = (sigma_p / sigma) * std::exp(-eta * h);
    c[4] = sigma_p * std::sqrt(-std::expm1(-2.0 * eta * h));
    if (solver == kSolverDpmpp2M) {
      if (order >= 1) {
        const double r = h_prev / h;
        c[1] = alpha_p * A * (1.0 + 1.0 / (2.0 * r));
        c[2] = -alpha_p * A / (2.0 * r);
      } else {
        c[1] = alpha_p * A;
        c[2] = 0.0;
      }
    } else {                     // kSolverDpmpp3M: k-diffusion's sample_dpmpp_3m_sde in alpha / sigma terms
      const double h_eta = (1.0 + eta) * h;
      const double phi2 = std::expm1(-h_eta) / h_eta + 1.0;
      if (order >= 2) {
        const double phi3 = phi2 / h_eta - 0.5;
        const double r0 = h_prev / h, r1 = h_prev2 / h;
        const double P = phi2 * (1.0 + r0 / (r0 + r1)) - phi3 / (r0 + r1), Q = (phi3 - phi2 * r0) / (r0 + r1);
        c[1] = alpha_p * (A + P / r0);
        c[2] = alpha_p * (-P / r0 + Q / r1);
        c[3] = -alpha_p * Q / r1;
      } else if (order == 1) {
        const double r0 = h_prev / h;
        c[1] = alpha_p * (A + phi2 / r0);
        c[2] = -alpha_p * phi2 / r0;
      } else {
        c[1] = alpha_p * A;
        c[2] = 0.0;
      }
    }
    h_prev2 = h_prev;
    h_prev = h;
    order = std::min(order + 1, 2);
  }
}

const char* Diffuser::explicit_noise_error(const double* alphas, int n_train, const Schedule& sc, int solver, int prediction) {
  if (!solver_is_row1(solver)) return nullptr;      // DDIM, 2M and 3M at eta == 0 draw nothing
  std::vector<double> rows((size_t)kRowCols * sc.size());
  solver_coefficients(alphas, n_train, sc, solver, 0.0, rows.data(), prediction);
  for (size_t i = 0; i < sc.size(); ++i)
    if (rows[kRowCols * i + 4] != 0.0)
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
  for (void* p : {(void*)table_, (void*)active_, (void*)moments_, (void*)factors_, (void*)step_idx_, (void*)t_dev_, (void*)hist_, (void*)hist2_})
    if (p) (void)hipFree(p);
}

int StepLoop::begin(const std::vector<double>& alphas, const Schedule& sc, int solver, double eta, double cfg_scale,
                    const Guidance& go, bool single, int n, int HW, const StepIo& io, hipStream_t s, int prediction) {
  const int n_train = (int)alphas.size();
  SDXL_REQUIRE(n >= 1 && n <= kMaxSeeds, "batch out of range");
  // a == 0 on an iteration: x0 = -v under kPredictionV; under kPredictionEpsilon the first update would divide by sqrt_a == 0
  if (const char* m = Diffuser::schedule_error(sc, prediction)) throw InvalidArgumentError(m);
  SDXL_REQUIRE(single || go.n_scales == 0 || go.n_scales == n, "guidance: n_scales differs from the batch (cond.n)");
  const bool rows = solver != kSolverDdim;             // the 2M layout of the table: 2M itself and the first-order rows of LCM / TCD
  if (!io.seeds)
    if (const char* m = Diffuser::explicit_noise_error(alphas.data(), n_train, sc, solver, prediction)) throw InvalidArgumentError(m);
  // --- coefficient table (host f64, exactly the reference's scalar arithmetic :407-414, :423-426)
  const int iters = (int)sc.size();
  std::vector<StepCoef> tab(iters + 1);
  act_.assign(iters, 1);                               // guidance interval: iteration i is active where t_lo <= t_i <= t_hi
  std::vector<double> c2m;
  if (rows) {
    c2m.resize((size_t)kRowCols * iters);
    Diffuser::solver_coefficients(alphas.data(), n_train, sc, solver, eta, c2m.data(), prediction);
  }
  for (int i = 0; i < iters; ++i) {
    const double t = sc.t[i];
    const double a = sc.a[i];
    const double ap = sc.ap(i);
    StepCoef k{};
    k.t = (float)t;
    k.sqrt_a = (float)std::sqrt(a);
    k.sqrt_1ma = (float)std::sqrt(1.0 - a);
    if (rows) {
      const double* c = &c2m[(size_t)kRowCols * i];
      k.c_x = (float)c[0]; k.c_0 = (float)c[1]; k.c_1 = (float)c[2]; k.c_2 = (float)c[3]; k.c_z = (float)c[4];
    } else {
      double sqrt_ap, sqrt_1map, sigma;
      ddim_terms(a, ap, eta, sqrt_ap, sqrt_1map, sigma);
      k.sqrt_ap = (float)sqrt_ap;
      k.sqrt_1map = (float)sqrt_1map;
      k.sigma = (float)sigma;
    }
    tab[i] = k;
    if (!single) act_[i] = t >= (double)go.t_lo && t <= (double)go.t_hi;
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
  if (solver == kSolverDpmpp2M || solver == kSolverDpmpp3M) ensure_device(hist_, hist_cap_, (size_t)n * 4 * HW);      // kSolverRow1 keeps no history: nothing is allocated
  if (solver == kSolverDpmpp3M) ensure_device(hist2_, hist2_cap_, (size_t)n * 4 * HW);
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
  p_.hist2 = solver == kSolverDpmpp3M ? hist2_ : nullptr;
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
void Diffuser::diffuse(float* latent, const Conditioning& c, const Schedule& sc, double cfg_scale,
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

  const int iters = loop_.begin(alphas_, sc, solver_, eta, cfg_scale, go, single, n, HW, io, s, prediction_);
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
  const Schedule sc = call_schedule(n_steps, t.step_start, t.renoise != nullptr, t.start != nullptr);
  if (const char* m = schedule_error(sc, prediction_)) throw InvalidArgumentError(m);
  if (solver_ == kSolverLcm && t.eta != 0.0) throw InvalidArgumentError("solver LCM takes no eta: eta must be 0 (SDXL_SOLVER_LCM)");
  if (solver_ == kSolverTcd && sc.from_sigmas)
    throw InvalidArgumentError("solver TCD reads alphas_cumprod at floor((1 - gamma) t'), a training timestep: it does not run on sigmas (use a timestep list)");
  if (!t.seeds)
    if (const char* m = explicit_noise_error(alphas_.data(), n_train_, sc, solver_, prediction_)) throw InvalidArgumentError(m);
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
  } else if (t.start) {
    if (t.renoise0) {           // continue_latent with renoise: to the list's own first level
      const float* noise = t.noise;
      if (!noise) {
        ensure_device(noise_, noise_cap_, elems);
        launch_seeded_noise(noise_, t.seeds, kDrawInitial, c.n, HW, s);
        noise = noise_;
      }
      const double a = sc.a[0];
      launch_axpby(latent_, t.start, (float)std::sqrt(a), noise, (float)std::sqrt(1.0 - a), elems, s);
    } else {
      SDXL_HIP(hipMemcpyAsync(latent_, t.start, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  } else if (t.seeds) {
    launch_seeded_noise(latent_, t.seeds, kDrawInitial, c.n, HW, s);
  } else {
    SDXL_HIP(hipMemcpyAsync(latent_, t.noise, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  diffuse(latent_, c, sc, cfg_scale, t.reference, t.mask, t.step_noise, s, t.seeds, t.eta);
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

void Diffuser::continue_latent(const float* latent, const Conditioning& c, double cfg_scale, int n_steps, const float* noise, const uint64_t* seeds,
                               double eta, bool renoise, float* out, hipStream_t s) {
  SDXL_REQUIRE(latent && out, "null argument");
  if (renoise && (noise != nullptr) == (seeds != nullptr))
    throw InvalidArgumentError("continue_latent: renoise takes exactly one of noise (an explicit tensor) and seeds (the SDXL_DRAW_INITIAL draw)");
  if (!seeds && eta != 0.0) throw InvalidArgumentError("eta needs seeds: explicit noise carries none for the sigma term");
  Trajectory t; t.start = latent; t.renoise0 = renoise; t.noise = renoise ? noise : nullptr; t.seeds = seeds; t.eta = eta;
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
