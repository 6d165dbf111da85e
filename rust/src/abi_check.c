/* compile-time pins of the C ABI the Rust shim relies on (built by build.rs with `cc`) */
#include "sdxl_mi355.h"
_Static_assert(SDXL_OK == 0, "status code");
_Static_assert(SDXL_DTYPE_F32 == 0 && SDXL_DTYPE_F16 == 1 && SDXL_DTYPE_F16_F32RES == 2 && SDXL_DTYPE_F32_SPLIT == 3 && SDXL_DTYPE_F32_SPLIT_MIX == 4 && SDXL_DTYPE_F32_SPLIT_MIX_F16W == 5 && SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2 == 6 && SDXL_DTYPE_F32_SPLIT_F16W == 7, "dtype codes");
_Static_assert(sizeof(sdxl_conditioning) == 8 * sizeof(void*) + 4 * sizeof(int32_t), "sdxl_conditioning layout");
#include <stddef.h>
_Static_assert(SDXL_LORA_ROUND_F16 == 1, "lora flags");
_Static_assert(offsetof(sdxl_lora_entry, param_index) == 0 && offsetof(sdxl_lora_entry, rank) == 4 && offsetof(sdxl_lora_entry, left) == 8 &&
               offsetof(sdxl_lora_entry, right) == 8 + sizeof(void*) && offsetof(sdxl_lora_entry, scale) == 8 + 2 * sizeof(void*) &&
               sizeof(sdxl_lora_entry) == 16 + 2 * sizeof(void*), "sdxl_lora_entry layout (LP64)");
_Static_assert(SDXL_GUIDANCE_CFG == 0 && SDXL_GUIDANCE_OFF == 1, "guidance modes");
_Static_assert(offsetof(sdxl_guidance, mode) == 0 && offsetof(sdxl_guidance, rescale) == 4 && offsetof(sdxl_guidance, n_scales) == 8 &&
               offsetof(sdxl_guidance, scales) == 12 && offsetof(sdxl_guidance, t_lo) == 44 && offsetof(sdxl_guidance, t_hi) == 48 &&
               sizeof(sdxl_guidance) == 52, "sdxl_guidance layout");
_Static_assert(offsetof(sdxl_control, scale) == 0 && offsetof(sdxl_control, n_scales) == 4 && offsetof(sdxl_control, scales) == 8 &&
               offsetof(sdxl_control, t_lo) == 40 && offsetof(sdxl_control, t_hi) == 44 && offsetof(sdxl_control, cond_only) == 48 &&
               sizeof(sdxl_control) == 52, "sdxl_control layout");
_Static_assert(SDXL_SOLVER_DDIM == 0 && SDXL_SOLVER_DPMPP_2M == 1 && SDXL_SOLVER_LCM == 3 && SDXL_SOLVER_TCD == 4, "solver codes");
_Static_assert(SDXL_SCHEDULE_REFERENCE == 0 && SDXL_SCHEDULE_TRAILING == 1 && SDXL_SCHEDULE_LEADING == 2 && SDXL_SCHEDULE_LCM == 3, "timestep schedule kinds");
_Static_assert(SDXL_MAX_CONTROLS == 4, "control nets per handle");
_Static_assert(SDXL_SOLVER_DPMPP_3M == 5 && SDXL_SIGMAS_ROUND_T == 1 && SDXL_SIGMAS_KARRAS == 0 && SDXL_SIGMAS_EXPONENTIAL == 1 && SDXL_SIGMAS_OF_TIMESTEPS == 2,
               "noise-level codes");
_Static_assert(offsetof(sdxl_schedule_desc, alphas_cumprod_host) == 0 && offsetof(sdxl_schedule_desc, n_train_steps) == sizeof(void*) &&
               offsetof(sdxl_schedule_desc, timesteps) == 2 * sizeof(void*) && offsetof(sdxl_schedule_desc, sigmas) == 3 * sizeof(void*) &&
               offsetof(sdxl_schedule_desc, n) == 4 * sizeof(void*) && offsetof(sdxl_schedule_desc, t_end) == 4 * sizeof(void*) + 4 &&
               offsetof(sdxl_schedule_desc, sigma_end) == 4 * sizeof(void*) + 8 && offsetof(sdxl_schedule_desc, flags) == 4 * sizeof(void*) + 16 &&
               sizeof(sdxl_schedule_desc) == 4 * sizeof(void*) + 24, "sdxl_schedule_desc layout (LP64)");
int sdxl_mi355_abi_check(void) { return SDXL_OK; }
