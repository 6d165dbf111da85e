// The launch descriptions of sdxl_debug_igemm_select / sdxl_debug_attn_select (include/sdxl_mi355.h) as the parameter blocks the
// selection reads.  Plain host C++: the entries in capi.hip and the stand-alone sanitizer driver (tests/select_driver.cpp) share it.
// Operand pointers are made-up addresses -- the selection reads them for null-ness and alignment only.
#pragma once
#include "kernels.h"
#include "../../include/sdxl_mi355.h"

namespace sdxl {

inline SelectKnobs select_debug_knobs(const sdxl_select_knobs& k) {
  SelectKnobs s;
  s.igemm_variant = k.igemm_variant; s.igemm_wreg = k.igemm_wreg; s.wreg_xattn = k.wreg_xattn; s.hl_tile96 = k.hl_tile96; s.igemm_tsw = k.igemm_tsw;
  s.igemm_unrolled = k.igemm_unrolled; s.wide_db = k.wide_db; s.attn_variant = k.attn_variant; s.attn_xsplit = k.attn_xsplit; s.zero_page = k.zero_page;
  return s;
}
inline void* select_debug_ptr(int slot, int misaligned) { return reinterpret_cast<void*>(((uintptr_t)(slot + 1) << 20) + (misaligned ? 8 : 0)); }

inline IgemmParams select_debug_igemm(const sdxl_igemm_case& c) {
  auto ptr = [&](int slot, unsigned bit) { return !bit || (c.present & bit) ? select_debug_ptr(slot, c.misaligned) : nullptr; };
  IgemmParams p{};
  int side = 1;
  while (side * side < c.rows_per_entry) ++side;
  p.Hout = side * side == c.rows_per_entry ? side : c.rows_per_entry;
  p.Wout = side * side == c.rows_per_entry ? side : 1;
  p.B = c.batch; p.ksize = c.ksize; p.stride = c.stride; p.pad = c.ksize / 2; p.up = c.up;
  p.Hin = (p.Hout * c.stride) >> c.up; p.Win = (p.Wout * c.stride) >> c.up;
  p.Cin = c.cin; p.lda = c.cin; p.a_dt = c.a_dt;
  p.M = c.batch * c.rows_per_entry; p.N = c.N; p.K = c.ksize * c.ksize * c.cin;
  const int kt = c.compute_dt == DT_F16 ? 64 : 32;
  p.Kpad = (p.K + kt - 1) / kt * kt;
  p.rpb = c.rows_per_entry; p.act = c.act;
  p.A = ptr(0, 0); p.W = ptr(1, 0); p.Wf = ptr(2, SDXL_SEL_WF);
  p.bias = static_cast<const float*>(ptr(3, 0));
  p.ebias = static_cast<const float*>(ptr(4, SDXL_SEL_EBIAS)); p.ebias_ld = c.N;
  p.C = ptr(5, 0); p.c_dt = c.c_dt; p.ldc = c.act == 1 ? c.N / 2 : c.N;
  p.R = ptr(6, SDXL_SEL_R); p.ldr = p.ldc; p.r_dt = c.c_dt;
  p.n_split = c.n_split >= 0 ? c.n_split : c.N;
  if (c.n_split >= 0) { p.Ct = ptr(7, 0); p.ct_rows = c.N - c.n_split; p.ct_ld = (c.rows_per_entry + 63) / 64 * 64; }
  p.ln_stat = static_cast<const float*>(ptr(8, SDXL_SEL_LN_STAT)); p.ln_slots = p.K / 64; p.ln_cs = p.ln_stat; p.ln_invc = 1.0f / (float)p.K; p.ln_eps = 1e-5f;
  p.stat_out = static_cast<float*>(ptr(9, SDXL_SEL_STAT_OUT)); p.stat_slots = c.N / 64;
  p.splitk_ws = static_cast<float*>(ptr(10, SDXL_SEL_SPLITK_WS)); p.splitk_cnt = static_cast<unsigned*>(ptr(11, SDXL_SEL_SPLITK_WS));
  p.splitk_ws_bytes = p.splitk_ws ? ~(size_t)0 >> 1 : 0;
  p.xa_k = ptr(12, SDXL_SEL_XA_K); p.xa_k_lo = ptr(13, SDXL_SEL_XA_K_LO); p.xa_nctx = c.xa_nctx; p.xa_scale = 0.125f;
  p.gn_part = static_cast<float*>(ptr(14, SDXL_SEL_GN_PART));
  p.acc_scale = static_cast<const float*>(ptr(15, SDXL_SEL_ACC_SCALE));
  p.shadow = ptr(16, SDXL_SEL_SHADOW);
  if (p.shadow) { p.shadow_gamma = static_cast<const float*>(ptr(17, 0)); p.shadow_ld = c.shadow_lo_sign > 0 ? 2 * c.N : c.N; p.shadow_lo_scale = 4096.0f * c.shadow_lo_sign; }
  if (c.present & SDXL_SEL_WARM) { p.warm[0] = ptr(18, 0); p.warm_bytes[0] = 1u << 20; }
  return p;
}

inline AttnParams select_debug_attn(const sdxl_attn_case& c) {
  AttnParams p{};
  p.B = c.B; p.H = c.H; p.Nq = c.Nq; p.Nk = c.Nk; p.dt = c.dt; p.scale = 0.125f;
  p.Q = select_debug_ptr(0, c.misaligned); p.K = select_debug_ptr(1, c.misaligned); p.Vt = select_debug_ptr(2, c.misaligned); p.O = select_debug_ptr(3, c.misaligned);
  p.ldq = p.ldk = p.ldo = c.H * 64; p.vt_ld = (c.Nk + 63) / 64 * 64;
  if (c.present & SDXL_SEL_MASK) { p.mask = static_cast<const float*>(select_debug_ptr(4, 0)); p.ldmask = c.Nk; }
  if (c.present & SDXL_SEL_XSPLIT_WS) { p.xws = static_cast<float*>(select_debug_ptr(5, 0)); p.xcnt = static_cast<unsigned*>(select_debug_ptr(6, 0)); }
  return p;
}

}  // namespace sdxl
