// What the two translation units of the C ABI share: capi.hip (contexts, model handles, sampling, VAE) and capi_ops.hip
// (single-op and micro-benchmark entries).  Handles, status / error reporting, dtype mapping, scoped device scratch.
#pragma once
#include "../../include/sdxl_mi355.h"
#include "engine.h"

struct sdxl_ctx { int device = 0; hipStream_t stream = nullptr; };
struct sdxl_unet { sdxl_ctx* ctx = nullptr; sdxl::UNet* u = nullptr; bool owned = true; };
struct sdxl_diffuser { sdxl_ctx* ctx = nullptr; sdxl::Diffuser* d = nullptr; sdxl_unet view; };
struct sdxl_controlnet { sdxl_ctx* ctx = nullptr; sdxl::UNet* c = nullptr; ~sdxl_controlnet() { delete c; } };      // a UNet in control mode
struct sdxl_vae { sdxl_ctx* ctx = nullptr; sdxl::Vae* v = nullptr; };
struct sdxl_clip { sdxl_ctx* ctx = nullptr; sdxl::ClipText* c = nullptr; };

namespace sdxl {
extern thread_local std::string g_err;      // text behind sdxl_last_error(): one object, defined in capi.hip
inline int fail(int code, const std::string& m) { g_err = m; return code; }
#define API_BEGIN try {
#define API_END                                                              \
  return SDXL_OK;                                                            \
  } catch (const sdxl::InvalidArgumentError& e) { return fail(SDXL_ERR_INVALID, e.what()); } \
  catch (const sdxl::Error& e) { return fail(SDXL_ERR_RUNTIME, e.what()); } \
  catch (const std::exception& e) { return fail(SDXL_ERR_RUNTIME, e.what()); } \
  catch (...) { return fail(SDXL_ERR_RUNTIME, "unknown error"); }

inline hipStream_t pick(sdxl_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }
inline void use(sdxl_ctx* c) { SDXL_HIP(hipSetDevice(c->device)); }

inline void no_mix(int dtype) {     // the mixed mode is a property of the UNet driver (which classes run in f16): UNet / Diffuser handles only
  if (dtype == SDXL_DTYPE_F32_SPLIT_MIX || dtype == SDXL_DTYPE_F32_SPLIT_MIX_F16W || dtype == SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2 || dtype == SDXL_DTYPE_F32_SPLIT_F16W) throw Error("SDXL_DTYPE_F32_SPLIT_MIX* are UNet / Diffuser modes (use SDXL_DTYPE_F32_SPLIT here)");
}
inline int mix_of(int dtype) {
  return dtype == SDXL_DTYPE_F32_SPLIT_MIX ? (MIX_ATTN_F16 | MIX_GEGLU_F16 | MIX_GEGLU_HILO)      // (round 6: GEGLU weights as (hi, lo) pairs along K -- activation rounding only on any weights)
       : dtype == SDXL_DTYPE_F32_SPLIT_MIX_F16W ? (MIX_ATTN_F16 | MIX_GEGLU_F16 | MIX_QKV_F16 | MIX_FF_F16 | MIX_OUT1_F16 | MIX_OUT2_F16 | MIX_Q2_F16 | MIX_LN_SHADOW | MIX_XATTN_SPLIT)
       : dtype == SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2 ? (MIX_ATTN_F16 | MIX_GEGLU_F16 | MIX_QKV_F16 | MIX_FF_F16 | MIX_OUT1_F16 | MIX_OUT2_F16 | MIX_Q2_F16 | MIX_LN_SHADOW | MIX_XATTN_SPLIT | MIX_GEGLU_AHILO)
       : dtype == SDXL_DTYPE_F32_SPLIT_F16W ? (MIX_LINEAR_F16X2 | MIX_XATTN_SPLIT | MIX_LN_SHADOW) : 0;      // (no class on f16 OPERANDS: fp32-class arithmetic on the f16 kernels)
       // (round 6: + the cross-attention query projection on f16 with an fp32 q, the split-precision 77-key attention inside its epilogue, and the LayerNorms in
       //  front of the f16 projections folded through the f16 shadow of the stream -- DESIGN 4.1; MIX_XATTN_F16 stays a knob: DESIGN 11.2b)
}
inline void dtypes(int dtype, int& cdt, int& sdt) {
  switch (dtype) {
    case SDXL_DTYPE_F32: cdt = DT_F32; sdt = DT_F32; break;
    case SDXL_DTYPE_F16: cdt = DT_F16; sdt = DT_F16; break;
    case SDXL_DTYPE_F16_F32RES: cdt = DT_F16; sdt = DT_F32; break;
    case SDXL_DTYPE_F32_SPLIT: cdt = DT_HL; sdt = DT_F32; break;   // UNet / Diffuser / VAE only (no_split() guards the rest)
    case SDXL_DTYPE_F32_SPLIT_MIX: case SDXL_DTYPE_F32_SPLIT_MIX_F16W: case SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2: case SDXL_DTYPE_F32_SPLIT_F16W: cdt = DT_HL; sdt = DT_F32; break;   // UNet / Diffuser only (mix_of() carries the f16 classes)
    default: throw Error("unknown dtype");
  }
}
inline void no_split(int cdt, const char* what) {
  if (cdt == DT_HL) throw Error(std::string("SDXL_DTYPE_F32_SPLIT is not available for ") + what);
}
inline void vae_dtype(int dtype, int& cdt) {     // the VAE additionally takes the split-operand fp32-class mode
  int sdt;
  if (dtype == SDXL_DTYPE_F32_SPLIT) { cdt = DT_HL; return; }
  no_mix(dtype); dtypes(dtype, cdt, sdt);
}
struct Tmp {   // scoped device scratch for the single-op entry points
  std::vector<void*> ptrs;
  ~Tmp() { for (void* p : ptrs) (void)hipFree(p); }
  void* get(size_t bytes) { void* p = nullptr; SDXL_HIP(hipMalloc(&p, bytes ? bytes : 16)); ptrs.push_back(p); return p; }
};
// the single-op entry points run the same kernel selection as the models, split-K included (f16 compute only)
inline void give_splitk_ws(Exec& ex, Tmp& tmp, int batch, int rows_per_entry, int n, hipStream_t s) {
  if (ex.cdt != DT_F16) return;
  ex.splitk_ws_bytes = igemm_splitk_ws_bytes(batch, rows_per_entry, n);
  ex.splitk_ws = (float*)tmp.get(ex.splitk_ws_bytes);
  ex.splitk_cnt = (unsigned*)tmp.get(kSplitkCounters * sizeof(unsigned));
  SDXL_HIP(hipMemsetAsync(ex.splitk_cnt, 0, kSplitkCounters * sizeof(unsigned), s));
}
}  // namespace sdxl
