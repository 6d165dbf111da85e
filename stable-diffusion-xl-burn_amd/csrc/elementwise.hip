// Small HBM-/launch-bound kernels of the SDXL hot path for gfx950: GEMV (M<=8 linears), row softmax (unfused
// attention path), sinusoidal timestep embedding, layout conversion at the NCHW API boundary, the fused
// CFG-combine + DDIM update, image <-> activation conversion, synthetic weight fill and weight packing.
#include "kernels.h"
#include "upsample_fold.h"
#include <algorithm>
#include <stdexcept>

namespace sdxl {

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// DT_HL (split-operand storage "HL16", kernels.h): logical element i of a tensor whose rows are multiples of 16 elements lives as
// hi = f16(v) at half index (i/16)*32 + i%16 and lo = f16(v - hi) 16 halfs further
__device__ __forceinline__ float ld_f(const void* p, size_t i, int dt) {
  if (dt == DT_HL) { const half_t* b = reinterpret_cast<const half_t*>(p) + ((i >> 4) << 5) + (i & 15); return (float)b[0] + (float)b[16]; }
  return dt == DT_F16 ? (float)reinterpret_cast<const half_t*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ void st_f(void* p, size_t i, int dt, float v) {
  if (dt == DT_HL) {
    half_t* b = reinterpret_cast<half_t*>(p) + ((i >> 4) << 5) + (i & 15);
    const half_t hi = (half_t)v;
    b[0] = hi; b[16] = (half_t)(v - (float)hi);
  } else if (dt == DT_F16) reinterpret_cast<half_t*>(p)[i] = (half_t)v; else reinterpret_cast<float*>(p)[i] = v;
}
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------
// GEMV: Bm (<= 8) input rows against a packed [N][Kpad] weight: the block first parks the inputs in LDS -- SiLU applied ONCE
// per block when requested -- then each of its 4 wavefronts walks `cols` output columns (4 for wide outputs, 1 when N is small and the grid would not fill the chip), streaming the weights once with
// 16-byte loads.  (Round 1 had every wavefront re-read x from global and re-evaluate silu(x) per output column: the
// lin_embed(silu(emb)) projection of all ResBlocks, 14 k columns x 1280 inputs, spent 76 us per step on 35 M redundant expf.)
// (time / label embedding MLPs unet/mod.rs:458-468 and the ResBlock lin_embed(silu(emb)) :1088-1089)
template <typename WT>
__global__ __launch_bounds__(256) void gemv_kernel(const GemvParams p, int cols) {
  constexpr int CE = 16 / sizeof(WT);
  extern __shared__ __attribute__((aligned(16))) float gx[];      // [Bm][Kx], Kx = K rounded up to 64 * CE (zero tail)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Kx = (p.K + 64 * CE - 1) / (64 * CE) * (64 * CE);
  for (int i = threadIdx.x; i < p.Bm * Kx; i += 256) {
    const int b = i / Kx, k = i - b * Kx;
    float x = 0.f;
    if (k < p.K) {
      x = p.X[(size_t)b * p.ldx + k];
      if (p.silu_in) x = silu_f(x);
    }
    gx[i] = x;
  }
  __syncthreads();
  const int n0 = (blockIdx.x * 4 + wave) * cols;
  for (int c = 0; c < cols; ++c) {
    const int n = n0 + c;
    if (n >= p.N) return;                          // wave-uniform
    const WT* w = reinterpret_cast<const WT*>(p.W) + (size_t)n * p.Kpad;
    float acc[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[b] = 0.f;
    for (int k0 = lane * CE; k0 < p.K; k0 += 64 * CE) {
      float wv[CE];
      if constexpr (sizeof(WT) == 2) {
        half8 h = *reinterpret_cast<const half8*>(w + k0);
#pragma unroll
        for (int j = 0; j < CE; ++j) wv[j] = (float)h[j];
      } else {
        f32x4 f = *reinterpret_cast<const f32x4*>(w + k0);
#pragma unroll
        for (int j = 0; j < CE; ++j) wv[j] = f[j];
      }
      // weight columns k >= K of the zero-padded row meet the zero tail of gx: no bounds test in the inner loop
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b < p.Bm) {
          const float* xr = gx + b * Kx + k0;
#pragma unroll
          for (int j = 0; j < CE; j += 4) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + j);
            acc[b] += xv[0] * wv[j] + xv[1] * wv[j + 1] + xv[2] * wv[j + 2] + xv[3] * wv[j + 3];
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[b] += __shfl_xor(acc[b], o);
    }
    if (lane == 0) {
      for (int b = 0; b < p.Bm; ++b) {
        float v = acc[b] + (p.bias ? p.bias[n] : 0.f);
        if (p.silu_out) v = silu_f(v);
        if (p.Yadd) v += p.Yadd[(size_t)b * p.ldy + n];
        p.Y[(size_t)b * p.ldy + n] = v;
      }
    }
  }
}
void launch_gemv(const GemvParams& pin, hipStream_t s) {
  const int ce = pin.w_dt == DT_F16 ? 8 : 4;
  const int Kx = (pin.K + 64 * ce - 1) / (64 * ce) * (64 * ce);
  const size_t row_bytes = (size_t)Kx * sizeof(float);
  if (row_bytes > 64 * 1024) throw std::runtime_error("gemv: K does not fit the 64 KiB input staging buffer");
  const int rows_per_launch = (int)std::min<size_t>(8, (64 * 1024) / row_bytes);     // e.g. K = 2816 (label MLP): 5 rows per launch
  for (int b0 = 0; b0 < pin.Bm; b0 += rows_per_launch) {
    GemvParams p = pin;
    p.Bm = std::min(rows_per_launch, pin.Bm - b0);
    p.X = pin.X + (size_t)b0 * pin.ldx;
    p.Y = pin.Y + (size_t)b0 * pin.ldy;
    if (pin.Yadd) p.Yadd = pin.Yadd + (size_t)b0 * pin.ldy;
    const size_t lds = (size_t)p.Bm * row_bytes;
    const int cols = p.N >= 8192 ? 4 : 1;
    dim3 g((p.N + 4 * cols - 1) / (4 * cols));
    if (p.w_dt == DT_F16) hipLaunchKernelGGL(gemv_kernel<half_t>, g, dim3(256), lds, s, p, cols);
    else hipLaunchKernelGGL(gemv_kernel<float>, g, dim3(256), lds, s, p, cols);
  }
}

// ---------------------------------------------------------------------------------------------------------
// row softmax (one 256-thread block per row)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* S, int lds_, void* P, int p_dt, int ldp, int n,
                                                           int npad, float scale, const float* mask, int ldmask,
                                                           int mask_rows, float p_scale, float* p_scale_out) {
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* s = S + (size_t)row * lds_;
  const float* mk = mask ? mask + (size_t)(row % mask_rows) * ldmask : nullptr;
  float mx = -INFINITY;
  for (int i = tid; i < n; i += 256) mx = fmaxf(mx, s[i] * scale + (mk ? mk[i] : 0.f));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int i = tid; i < n; i += 256) sum += expf(s[i] * scale + (mk ? mk[i] : 0.f) - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = sum;
  __syncthreads();
  sum = red[4] + red[5] + red[6] + red[7];
  // p_scale (split-operand P V product, thousands of keys): probabilities ~1e-4 would put the lo halves of an HL16 P into the f16
  // subnormals -- P is stored times a power of two and the P V GEMM undoes it through its accumulator scale (p_scale_out[0])
  const float inv = p_scale / sum;
  if (p_scale_out && row == 0 && tid == 0) { p_scale_out[0] = 1.0f / p_scale; p_scale_out[1] = 0.f; }
  for (int i = tid; i < npad; i += 256) {
    const float v = i < n ? expf(s[i] * scale + (mk ? mk[i] : 0.f) - mx) * inv : 0.f;
    st_f(P, (size_t)row * ldp + i, p_dt, v);
  }
}
void launch_softmax_rows(const float* S, int lds_, void* P, int p_dt, int ldp, int rows, int n, int npad, float scale,
                         const float* mask, int ldmask, int mask_rows, hipStream_t s, float p_scale, float* p_scale_out) {
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, s, S, lds_, P, p_dt, ldp, n, npad, scale, mask,
                     ldmask, mask_rows > 0 ? mask_rows : 1, p_scale, p_scale_out);
}

// ---------------------------------------------------------------------------------------------------------
// timestep embedding, unet/mod.rs:21-39:  freqs = exp(arange(half) * (-ln(max_period)/half)); [cos | sin]
__global__ void temb_kernel(const float* t_dev, int t_stride, float* out, int Bm, int dim) {
  const int half = dim / 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bm * half) return;
  const int b = i / half, j = i - b * half;
  const float coef = (float)(-9.210340371976184 / (double)half);   // -ln(10000)/half rounded to f32 (burn: f64 scalar -> elem)
  const float f = expf((float)j * coef);
  const float a = t_dev[(size_t)b * t_stride] * f;
  out[(size_t)b * dim + j] = cosf(a);
  out[(size_t)b * dim + half + j] = sinf(a);
}
void launch_timestep_embedding(const float* t_dev, int t_stride, float* out, int Bm, int dim, hipStream_t s) {
  const int n = Bm * (dim / 2);
  hipLaunchKernelGGL(temb_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t_dev, t_stride, out, Bm, dim);
}

// conditioning_embedding (unet/mod.rs:41-57): out[b] = [pooled[b] | temb(vals[b][0]) | ... | temb(vals[b][w-1])]
__global__ void cond_embedding_kernel(const float* pooled, int E, const int* vals, int w, int dim, float* out, int n) {
  const int half = dim / 2;
  const int ld = E + w * dim;
  const int per = E + w * half;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * per) return;
  const int b = i / per, c = i - b * per;
  if (c < E) { out[(size_t)b * ld + c] = pooled[(size_t)b * E + c]; return; }
  const int v = (c - E) / half, j = (c - E) - v * half;
  const float coef = (float)(-9.210340371976184 / (double)half);
  const float a = (float)vals[b * w + v] * expf((float)j * coef);
  out[(size_t)b * ld + E + v * dim + j] = cosf(a);
  out[(size_t)b * ld + E + v * dim + half + j] = sinf(a);
}
void launch_conditioning_embedding(const float* pooled, int E, const int* vals, int w, int dim, float* out, int n, hipStream_t s) {
  const int total = n * (E + w * (dim / 2));
  hipLaunchKernelGGL(cond_embedding_kernel, dim3((total + 255) / 256), dim3(256), 0, s, pooled, E, vals, w, dim, out, n);
}

// ---------------------------------------------------------------------------------------------------------
__global__ void nchw_to_nhwc_kernel(const float* src, int sbs, void* dst, int dt, int B, int C, int HW, int ldd, float scale) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)B * HW * C;
  if (i >= total) return;
  const int c = i % C;
  const size_t pix = i / C;
  const int b = pix / HW;
  const int hw = pix - (size_t)b * HW;
  st_f(dst, pix * ldd + c, dt, src[(size_t)b * sbs + (size_t)c * HW + hw] * scale);
}
void launch_nchw_to_nhwc(const float* src, int sbs, void* dst, int dt, int B, int C, int HW, int ldd, float scale,
                         hipStream_t s) {
  const size_t total = (size_t)B * HW * C;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((total + 255) / 256), dim3(256), 0, s, src, sbs, dst, dt, B, C, HW, ldd, scale);
}
__global__ void nhwc_to_nchw_kernel(const void* src, int dt, int lds_, float* dst, int B, int C, int HW, float scale) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)B * HW * C;
  if (i >= total) return;
  const int hw = i % HW;
  const size_t bc = i / HW;
  const int c = bc % C;
  const int b = bc / C;
  dst[i] = ld_f(src, ((size_t)b * HW + hw) * lds_ + c, dt) * scale;
}
void launch_nhwc_to_nchw(const void* src, int dt, int lds_, float* dst, int B, int C, int HW, float scale, hipStream_t s) {
  const size_t total = (size_t)B * HW * C;
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((total + 255) / 256), dim3(256), 0, s, src, dt, lds_, dst, B, C, HW, scale);
}
__global__ void copy_rows_kernel(const void* src, int sdt, int lds_, void* dst, int ddt, int ldd, size_t rows, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C) return;
  const size_t r = i / C;
  const int c = i - r * C;
  st_f(dst, r * ldd + c, ddt, ld_f(src, r * lds_ + c, sdt));
}
void launch_copy_rows(const void* src, int sdt, int lds_, void* dst, int ddt, int ldd, int rows, int C, hipStream_t s) {
  const size_t total = (size_t)rows * C;
  hipLaunchKernelGGL(copy_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, s, src, sdt, lds_, dst, ddt, ldd, (size_t)rows, C);
}
__global__ void i32_to_f32_kernel(const int* src, float* dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (float)src[i];
}
void launch_i32_to_f32(const int* src, float* dst, int n, hipStream_t s) {
  hipLaunchKernelGGL(i32_to_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n);
}
void launch_fill_zero(void* p, size_t bytes, hipStream_t s) { (void)hipMemsetAsync(p, 0, bytes, s); }
// 8 channels per thread: two 16-byte loads -> hi / lo f16 octets, two 16-byte stores
__global__ void f32_to_hl_kernel(const float* src, int lds_, half_t* dst, int ldd, size_t rows, int C8) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C8) return;
  const size_t r = i / C8;
  const int c = (int)(i - r * C8) * 8;
  const float* sp = src + r * lds_ + c;
  const f32x4 a = *reinterpret_cast<const f32x4*>(sp), b = *reinterpret_cast<const f32x4*>(sp + 4);
  half8 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    hi[e] = (half_t)a[e]; lo[e] = (half_t)(a[e] - (float)hi[e]);
    hi[4 + e] = (half_t)b[e]; lo[4 + e] = (half_t)(b[e] - (float)hi[4 + e]);
  }
  half_t* dp = dst + r * 2 * (size_t)ldd + ((c >> 4) << 5) + (c & 15);
  *reinterpret_cast<half8*>(dp) = hi;
  *reinterpret_cast<half8*>(dp + 16) = lo;
}
// one flag per weight matrix: 1.0f while every scaled element is exactly one f16 value (the reference's records are f16:
// HalfPrecisionSettings, src/bin/sample/main.rs:37), 0.0f as soon as one is not
__global__ void f16_exact_kernel(const float* src, size_t n, float wscale, float* exact) {
  const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (size_t i = i0; i < n; i += stride) {
    float x = src[i] * wscale;
    asm("" : "+v"(x));
    bad |= (float)(half_t)x != x;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) *exact = 0.0f;        // (benign race: every writer stores the same value)
}
void launch_f16_exact(const float* src, size_t n, float wscale, float* exact, hipStream_t s, bool accumulate) {
  if (!accumulate) { const float one = 1.0f; (void)hipMemcpyAsync(exact, &one, sizeof(float), hipMemcpyHostToDevice, s); (void)hipStreamSynchronize(s); }
  if (n == 0) return;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(f16_exact_kernel, dim3(blocks), dim3(256), 0, s, src, n, wscale, exact);
}
// Range-safe conversion of an fp32 STREAM tensor (residual stream, VAE hidden state: magnitudes a model does not bound) into an HL16
// GEMM operand: hi = f16(x) overflows to inf beyond 65504 (-> NaN out of the three-MFMA product) and below 6e-5 the lo half falls
// into the f16 subnormals.  The tensor is therefore converted times the power of two 2^e that brings max|x| into [2^13, 2^14) -- exact,
// the same rule the weights use (WeightBuilder::hl_scale) -- and the consuming GEMM undoes it through IgemmParams::a_scale.
// Round 6: ONE FACTOR PER BATCH ENTRY (an entry's operand bits, hence its results, do not depend on its batch neighbours -- the guarantee the
// f16 engine always gave), and no atomics / memset: the first kernel leaves kHlAbsBlocks per-block maxima per entry (every launch rewrites all of
// them), every block of the second reduces its entry's partials in its prologue (512 bytes out of the L2) and block 0 of an entry writes 2^-e.
__global__ void absmax_rows_kernel(const float* src, int lds_, size_t rows_per_entry, int C4, float* partial) {
  const int b = blockIdx.y;
  const float* sb = src + (size_t)b * rows_per_entry * lds_;
  float m = 0.f;
  const size_t total = rows_per_entry * (size_t)C4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  // four independent 16-byte loads in flight per thread: one load per trip is latency-bound on the VAE's 0.1 - 1 GB tensors (128 workgroups per entry:
  // 456 us per pass at ~1 TB/s).  A maximum does not depend on the order it is taken in.
  for (; i + 3 * stride < total; i += 4 * stride) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const size_t j = i + u * stride, r = j / C4; v[u] = *reinterpret_cast<const f32x4*>(sb + r * lds_ + (j - r * C4) * 4); }
#pragma unroll
    for (int u = 0; u < 4; ++u) m = fmaxf(fmaxf(m, fmaxf(fabsf(v[u][0]), fabsf(v[u][1]))), fmaxf(fabsf(v[u][2]), fabsf(v[u][3])));
  }
  for (; i < total; i += stride) {
    const size_t r = i / C4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(sb + r * lds_ + (i - r * C4) * 4);
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  // (round 5 lesson: one atomicMax per wave on a single address serialised in the L2 -- 97 us per call; now no atomic at all)
  __shared__ float wmax[4];
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)b * kHlAbsBlocks + blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));     // (NaN inputs: fmaxf drops them -- nothing to rescue there)
}
__device__ __forceinline__ float hl_stream_scale(float absmax) {
  if (!(absmax > 0.f) || !(absmax < INFINITY)) return 1.f;            // all-zero or non-finite tensors: nothing to rescue
  int e;
  (void)frexpf(absmax, &e);                                          // absmax = m 2^e, m in [0.5, 1)
  e = 14 - e;
  e = e > 60 ? 60 : (e < -60 ? -60 : e);
  return ldexpf(1.0f, e);
}
__global__ void f32_to_hl_scaled_kernel(const float* src, int lds_, half_t* dst, int ldd, size_t rows_per_entry, int C8, const float* partial, float* inv_out) {
  const int b = blockIdx.y;
  // this entry's max|x|: kHlAbsBlocks partials, one or none per thread
  float m = threadIdx.x < kHlAbsBlocks ? partial[(size_t)b * kHlAbsBlocks + threadIdx.x] : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float wmax[4];
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  const float sc = hl_stream_scale(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) inv_out[b] = 1.0f / sc;
  if (i >= rows_per_entry * C8) return;
  const size_t r = i / C8 + (size_t)b * rows_per_entry;
  const int c = (int)(i % C8) * 8;
  const float* sp = src + r * lds_ + c;
  const f32x4 a = *reinterpret_cast<const f32x4*>(sp), bb = *reinterpret_cast<const f32x4*>(sp + 4);
  half8 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float x = a[e] * sc, y = bb[e] * sc;                             // (pinned in fp32 first: see store_hl8)
    asm("" : "+v"(x)); asm("" : "+v"(y));
    hi[e] = (half_t)x; lo[e] = (half_t)(x - (float)hi[e]);
    hi[4 + e] = (half_t)y; lo[4 + e] = (half_t)(y - (float)hi[4 + e]);
  }
  half_t* dp = dst + r * 2 * (size_t)ldd + ((c >> 4) << 5) + (c & 15);
  *reinterpret_cast<half8*>(dp) = hi;
  *reinterpret_cast<half8*>(dp + 16) = lo;
}
void launch_f32_to_hl_scaled(const void* src, int lds_, void* dst, int ldd, size_t rows, int C, float* scale_io, hipStream_t s, int nb, bool have_partials) {
  if ((C & 15) != 0 || (lds_ & 3) != 0 || (ldd & 15) != 0) throw std::runtime_error("f32_to_hl: C % 16 == 0 rows with aligned strides only");
  if (nb < 1 || rows % (size_t)nb != 0) throw std::runtime_error("f32_to_hl: rows must split evenly over the batch entries");
  static_assert(kHlAbsBlocks <= 256, "one partial per thread of the conversion block");
  const size_t rpe = rows / nb;
  if (!have_partials) hipLaunchKernelGGL(absmax_rows_kernel, dim3(kHlAbsBlocks, nb), dim3(256), 0, s, reinterpret_cast<const float*>(src), lds_, rpe, C / 4, scale_io);
  const size_t total = rpe * (size_t)(C / 8);
  hipLaunchKernelGGL(f32_to_hl_scaled_kernel, dim3((unsigned)((total + 255) / 256), nb), dim3(256), 0, s, reinterpret_cast<const float*>(src), lds_,
                     reinterpret_cast<half_t*>(dst), ldd, rpe, C / 8, scale_io, hl_scale_inv(scale_io, nb));
}
__global__ void f32_to_f16_pair_kernel(const float* src, int lds_, half_t* hi, half_t* lo, int ld16, size_t rows, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * (size_t)C) return;
  const size_t r = i / C;
  const int c = (int)(i - r * C);
  float x = src[r * lds_ + c];
  asm("" : "+v"(x));
  const half_t h = (half_t)x;
  hi[r * ld16 + c] = h;
  lo[r * ld16 + c] = (half_t)(x - (float)h);
}
void launch_f32_to_f16_pair(const float* src, int lds_, void* hi, void* lo, int ld16, size_t rows, int C, hipStream_t s) {
  const size_t total = rows * (size_t)C;
  if (!total) return;
  hipLaunchKernelGGL(f32_to_f16_pair_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, lds_, reinterpret_cast<half_t*>(hi),
                     reinterpret_cast<half_t*>(lo), ld16, rows, C);
}
void launch_f32_to_hl(const void* src, int lds_, void* dst, int ldd, size_t rows, int C, hipStream_t s) {
  if ((C & 15) != 0 || (lds_ & 3) != 0 || (ldd & 15) != 0) throw std::runtime_error("f32_to_hl: C % 16 == 0 rows with aligned strides only");
  const size_t total = rows * (size_t)(C / 8);
  hipLaunchKernelGGL(f32_to_hl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float*>(src), lds_,
                     reinterpret_cast<half_t*>(dst), ldd, rows, C / 8);
}
// debugging aid (SDXL_NAN_CHECK=1, eager forwards): counts the non-finite elements of a [rows][C] view (HL16 views: both halves of every element)
__global__ void count_nonfinite_kernel(const void* src, int dt, int lds_, size_t rows, int C, unsigned* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C) return;
  const size_t r = i / C;
  const int c = (int)(i - r * C);
  bool bad;
  if (dt == DT_HL) {
    const half_t* p = reinterpret_cast<const half_t*>(src) + r * 2 * (size_t)lds_ + ((c >> 4) << 5) + (c & 15);
    const float hi = (float)p[0], lo = (float)p[16];
    bad = !(fabsf(hi) < INFINITY) || !(fabsf(lo) < INFINITY);
  } else {
    const float v = ld_f(src, r * lds_ + c, dt);
    bad = !(fabsf(v) < INFINITY);
  }
  if (bad) atomicAdd(out, 1u);
}
unsigned count_nonfinite(const void* src, int dt, int lds_, size_t rows, int C, hipStream_t s) {
  static unsigned* dev = nullptr;
  if (!dev && hipMalloc((void**)&dev, sizeof(unsigned)) != hipSuccess) return 0;
  (void)hipMemsetAsync(dev, 0, sizeof(unsigned), s);
  const size_t total = rows * (size_t)C;
  if (total) hipLaunchKernelGGL(count_nonfinite_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dt, lds_, rows, C, dev);
  unsigned h = 0;
  (void)hipMemcpyAsync(&h, dev, sizeof(unsigned), hipMemcpyDeviceToHost, s);
  (void)hipStreamSynchronize(s);
  return h;
}
// f16 rows -> HL16 rows with zero lo halves (an f16 value IS its own hi half): the hand-over from an f16 kernel (the mixed mode's flash
// attention) to a split-operand GEMM.  C % 16 == 0, lds % 8 == 0, ldd % 16 == 0.
__global__ void f16_to_hl_kernel(const half_t* src, int lds_, half_t* dst, int ldd, size_t rows, int C8) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C8) return;
  const size_t r = i / C8;
  const int c = (int)(i - r * C8) * 8;
  const half8 hi = *reinterpret_cast<const half8*>(src + r * lds_ + c);
  half_t* dp = dst + r * 2 * (size_t)ldd + ((c >> 4) << 5) + (c & 15);
  *reinterpret_cast<half8*>(dp) = hi;
  *reinterpret_cast<half8*>(dp + 16) = half8{0, 0, 0, 0, 0, 0, 0, 0};
}
void launch_f16_to_hl(const void* src, int lds_, void* dst, int ldd, size_t rows, int C, hipStream_t s) {
  if ((C & 15) != 0 || (lds_ & 7) != 0 || (ldd & 15) != 0) throw std::runtime_error("f16_to_hl: C % 16 == 0 rows with aligned strides only");
  const size_t total = rows * (size_t)(C / 8);
  if (!total) return;
  hipLaunchKernelGGL(f16_to_hl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const half_t*>(src), lds_,
                     reinterpret_cast<half_t*>(dst), ldd, rows, C / 8);
}
// precision-frontier instrument (round 5, UNet "hl_demote" classes): the lo halves of an HL16 tensor set to zero -- the (hi, lo) GEMM that
// reads it then multiplies exactly the f16 rounding of every element, i.e. the f16 engine's operand arithmetic on the split engine's kernels
__global__ void hl_zero_lo_kernel(half_t* dst, int ldd, size_t rows, int C16) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C16) return;
  const size_t r = i / C16;
  half_t* dp = dst + r * 2 * (size_t)ldd + (size_t)(i - r * C16) * 32 + 16;
  const half8 z = half8{0, 0, 0, 0, 0, 0, 0, 0};
  *reinterpret_cast<half8*>(dp) = z;
  *reinterpret_cast<half8*>(dp + 8) = z;
}
void launch_hl_zero_lo(void* dst, int ldd, size_t rows, int C, hipStream_t s) {
  if ((C & 15) != 0 || (ldd & 15) != 0) throw std::runtime_error("hl_zero_lo: C % 16 == 0 rows with aligned strides only");
  const size_t total = rows * (size_t)(C / 16);
  if (!total) return;
  hipLaunchKernelGGL(hl_zero_lo_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<half_t*>(dst), ldd, rows, C / 16);
}
__global__ void round_f16_kernel(float* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (float)(half_t)p[i];
}
void launch_round_f16(float* p, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(round_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n);
}
// Create-time adapter merge (LoraSource, sdxl_lora_merge): W[rows][cols] += scale * left[rows][rank] @ right[rank][cols], fp32 in place.
// The arithmetic is fixed -- per element acc = 0; acc = fmaf(left[r][j], right[j][c], acc) for j ascending; w = fmaf(scale, acc, w) -- so two
// runs give the same bits whatever the grid, and a host bound follows.  A block owns a 16-row x 64-column tile: the lanes of a wave run along the
// columns (coalesced loads / stores of W and of the right panel, LDS reads of consecutive words), each thread carries 4 rows; the left row panel is
// read as a broadcast.  Both panels go through LDS in chunks of 32 ranks; the accumulators stay in registers across the chunks.
constexpr int kLoraRows = 16, kLoraCols = 64, kLoraRank = 32;
__global__ __launch_bounds__(256) void lora_merge_kernel(float* w, size_t rows, size_t cols, const float* left, const float* right, int rank, float scale,
                                                         unsigned col_tiles) {
  __shared__ float sl[kLoraRows][kLoraRank];
  __shared__ float sr[kLoraRank][kLoraCols];
  const size_t r0 = (size_t)(blockIdx.x / col_tiles) * kLoraRows, c0 = (size_t)(blockIdx.x % col_tiles) * kLoraCols;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < rank; k0 += kLoraRank) {
    const int jn = rank - k0 < kLoraRank ? rank - k0 : kLoraRank;      // (the last chunk may be partial: the loop below never reads past it)
    for (int e = threadIdx.x; e < kLoraRows * kLoraRank; e += 256) {
      const int r = e / kLoraRank, j = e % kLoraRank;
      sl[r][j] = (r0 + r < rows && j < jn) ? left[(r0 + r) * (size_t)rank + k0 + j] : 0.f;
    }
    for (int e = threadIdx.x; e < kLoraRank * kLoraCols; e += 256) {
      const int j = e / kLoraCols, c = e % kLoraCols;
      sr[j][c] = (j < jn && c0 + c < cols) ? right[(size_t)(k0 + j) * cols + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < jn; ++j) {
      const float b = sr[j][tx];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(sl[ty * 4 + i][j], b, acc[i]);
    }
    __syncthreads();
  }
  if (c0 + tx >= cols) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t r = r0 + ty * 4 + i;
    if (r < rows) { float* p = w + r * cols + c0 + tx; *p = fmaf(scale, acc[i], *p); }
  }
}
void launch_lora_merge(float* w, size_t rows, size_t cols, const float* left, const float* right, int rank, float scale, hipStream_t s) {
  if (!rows || !cols || rank < 1 || scale == 0.f) return;      // (scale 0 is the identity on every bit pattern of W, -0 and non-finite products included)
  const size_t col_tiles = (cols + kLoraCols - 1) / kLoraCols, tiles = col_tiles * ((rows + kLoraRows - 1) / kLoraRows);
  if (tiles > 0x7fffffffull) throw std::runtime_error("lora_merge: tensor too large for one launch");
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, s, w, rows, cols, left, right, rank, scale, (unsigned)col_tiles);
}

// ---------------------------------------------------------------------------------------------------------
// CLIP text-encoder glue (clip/mod.rs:99-105 embedding sum, :139-147 eot pooling, backend.rs attn_decoder_mask)
__global__ void embed_tokens_kernel(const int* ids, const void* tok, const void* pos, int w_dt, void* x, int x_dt, int ldx,
                                    size_t rows, int S, int C, int n_vocab) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C) return;
  const size_t r = i / C;
  const int c = i - r * C;
  int id = ids[r];
  id = id < 0 ? 0 : (id >= n_vocab ? n_vocab - 1 : id);   // ids are validated on the host; never read out of the table
  st_f(x, r * ldx + c, x_dt, ld_f(tok, (size_t)id * C + c, w_dt) + ld_f(pos, (size_t)(r % S) * C + c, w_dt));
}
void launch_embed_tokens(const int* ids, const void* tok, const void* pos, int w_dt, void* x, int x_dt, int ldx, int B, int S,
                         int C, int n_vocab, hipStream_t s) {
  const size_t total = (size_t)B * S * C;
  hipLaunchKernelGGL(embed_tokens_kernel, dim3((total + 255) / 256), dim3(256), 0, s, ids, tok, pos, w_dt, x, x_dt, ldx,
                     (size_t)B * S, S, C, n_vocab);
}
// one wavefront per sequence: (value, index) butterfly, ties resolved to the lower index (= first occurrence, like argmax)
__global__ __launch_bounds__(64) void argmax_rows_kernel(const int* ids, int* out, int S) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int bv = -2147483647 - 1, bi = 0x7fffffff;
  for (int t = lane; t < S; t += 64) {
    const int v = ids[(size_t)b * S + t];
    if (v > bv) { bv = v; bi = t; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(bv, o), oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) out[b] = bi;
}
void launch_argmax_rows(const int* ids, int* out, int B, int S, hipStream_t s) {
  hipLaunchKernelGGL(argmax_rows_kernel, dim3(B), dim3(64), 0, s, ids, out, S);
}
__global__ void gather_rows_kernel(const void* x, int x_dt, int ldx, const int* idx, int S, float* out, int B, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  out[i] = ld_f(x, ((size_t)b * S + idx[b]) * ldx + c, x_dt);
}
void launch_gather_rows(const void* x, int x_dt, int ldx, const int* idx, int S, float* out, int B, int C, hipStream_t s) {
  hipLaunchKernelGGL(gather_rows_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, x, x_dt, ldx, idx, S, out, B, C);
}
__global__ void causal_mask_fill_kernel(float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n) return;
  const int r = i / n, c = i - r * n;
  out[i] = c > r ? -INFINITY : 0.f;
}
void launch_causal_mask(float* out, int n, hipStream_t s) {
  hipLaunchKernelGGL(causal_mask_fill_kernel, dim3((n * n + 255) / 256), dim3(256), 0, s, out, n);
}

// ---------------------------------------------------------------------------------------------------------
// Seeded noise: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11), key = the batch entry's
// 64-bit seed (low, high), counter = (hw, draw, 0, 0).  One call is the four channel values of one latent pixel: two
// Box-Muller pairs from the four output words.  Both uniforms are 24-bit fractions, exact in fp32; ua is in (0, 1] so the
// logarithm is finite and |z| <= sqrt(48 ln 2).  Contraction is off so the stand-alone fill and the in-register draw of
// step_kernel round every product alike.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ void seeded_normal4(uint64_t seed, uint32_t hw, uint32_t draw, float z[4]) {
#pragma clang fp contract(off)
  uint32_t x[4];
  philox4x32_10(hw, draw, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float ua = (float)((x[2 * p] >> 8) + 1u) * 5.9604644775390625e-08f;   // * 2^-24, exact, (0, 1]
    const float ub = (float)(x[2 * p + 1] >> 8) * 5.9604644775390625e-08f;      // exact, [0, 1)
    const float r = sqrtf(-2.0f * logf(ua));
    const float theta = 6.283185307179586f * ub;
    float sn, cs;
    sincosf(theta, &sn, &cs);
    z[2 * p] = r * cs;
    z[2 * p + 1] = r * sn;
  }
}
__global__ void seeded_noise_kernel(float* out, DdimSeeds seeds, uint32_t draw, int n, int HW) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n * HW) return;
  const int b = i / HW;
  const int hw = i - (size_t)b * HW;
  float z[4];
  seeded_normal4(seeds.v[b], (uint32_t)hw, draw, z);
#pragma unroll
  for (int c = 0; c < 4; ++c) out[((size_t)b * 4 + c) * HW + hw] = z[c];
}
void launch_seeded_noise(float* out, const uint64_t* seeds, uint32_t draw, int n, int HW, hipStream_t s) {
  for (int b0 = 0; b0 < n; b0 += kMaxSeeds) {
    const int nb = std::min(kMaxSeeds, n - b0);
    DdimSeeds k{};
    for (int b = 0; b < nb; ++b) k.v[b] = seeds[b0 + b];
    const size_t total = (size_t)nb * HW;
    hipLaunchKernelGGL(seeded_noise_kernel, dim3((total + 255) / 256), dim3(256), 0, s, out + (size_t)b0 * 4 * HW, k, draw, nb, HW);
  }
}

// ---------------------------------------------------------------------------------------------------------
// The per-step kernel: CFG combine + DDIM or DPM-Solver++(2M) update + sigma noise + inpaint blend + next-UNet-input refresh, one thread per
// latent pixel.  stablediffusion/mod.rs:423-428 (update), :539-540 (CFG), :463-465 (mask_where blend).
// SEEDED = false: explicit noise, eta = 0 (step_noise tensor; sigma / c_z never read).  SEEDED = true: the blend noise of :463 and the
// gen_noise() * sigma term of :427 are drawn in registers from the entry's seed (never stored); z is drawn only where its coefficient != 0.
// Every rounding is written out -- contraction off, fmaf where a product is fused, correctly rounded division -- so the bits do not depend on
// how the text is compiled; tests/test_gpu_sampler_step.py replays a recorded matrix of cases and demands them:
//     e   = fma(ec - eu, scales[b], eu), then e * factors[b] under CFG rescale; e = ec without CFG and on an inactive iteration
//     x0  = fma(-e, sqrt_1ma, x) / sqrt_a
//   kSolverDdim:     x = x0 sqrt_ap + e sqrt_1map with the first product fused into the sum on channels 2 and 3 only (channels 0 and 1 round
//                    both products: that is how the update was first compiled, and a trajectory amplifies a last-bit change)
//   kSolverDpmpp2M:  acc = c_1 * x0p      (p.hist, read only where c_1 != 0: a first-order row never looks at the history, whatever it holds)
//                    acc = fma(x0, c_0, acc);  x = fma(x, c_x, acc);  p.hist = x0 -- with inpainting the one computed from the blended state.
//                    The last row is (c_x, c_0, c_1, c_z) = (0, 1, 0, 0): the result is x0 itself.
//   kSolverRow1:     acc = x0 * c_0;  x = fma(x, c_x, acc): a first-order row of the 2M layout (the LCM and TCD tables).  No history:
//                    p.hist is neither read nor written.
//   kSolverDpmpp3M:  acc = c_2 * x0pp     (p.hist2, read only where c_2 != 0)
//                    acc = fma(x0p, c_1, acc)   (p.hist, read only where c_1 != 0);  acc = fma(x0, c_0, acc);  x = fma(x, c_x, acc)
//                    then p.hist2 = x0p where x0p was read and p.hist = x0: the histories shift per element, in place.
//     x   = fma(z, sigma or c_z, x)       (SEEDED, coefficient != 0; z = seeded_normal4(seed, hw, draw_sigma(idx)))
//   the blend rounds both products.
// PRED = kPredictionV: the network's rows are v = alpha e - sigma x0.  The two guidance lines above combine them as they combine e (v = vc;
// v = fma(vc - vu, scales[b], vu), then v * factors[b]), and the x0 line is replaced by
//     x0  = fma(x, sqrt_a, -(v * sqrt_1ma))           no division: finite at sqrt_a == 0 (zero terminal SNR), where x0 = -v
//     e   = fma(v, sqrt_a, x * sqrt_1ma)              kSolverDdim only; kSolverDpmpp2M never forms e
// with everything behind x0 and e the text of that solver.  The kPredictionEpsilon instantiations compile from the lines they always had.
template <int SOLVER, bool SEEDED, int PRED>
__global__ void step_kernel(const StepParams p, int do_update) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)p.n * p.HW) return;
  const int b = i / p.HW;
  const int hw = i - (size_t)b * p.HW;
  const int idx = *p.step_idx;
  const int next = do_update ? idx + 1 : 0;
  float x[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) x[c] = p.latent[((size_t)b * 4 + c) * p.HW + hw];
  if (do_update) {
    const StepCoef k = p.table[idx];
    const bool active = p.use_cfg && (!p.active || p.active[idx] != 0);     // uniform over the launch, as is whether p.factors is set
    // b is per lane (an entry boundary falls inside a wave wherever HW % 64 != 0).  The scale is selected from the eight argument words, which
    // arrive through scalar loads with the other arguments; indexing the by-value array with b made it a vector load from the argument
    // segment in front of the CFG line
    float sb = p.scales.v[0];
#pragma unroll
    for (int j = 1; j < kMaxSeeds; ++j) sb = b == j ? p.scales.v[j] : sb;
    const float fb = active && p.factors ? p.factors[b] : 1.f;
    float x0p[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SOLVER == kSolverDpmpp2M) {
      if (k.c_1 != 0.f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) x0p[c] = p.hist[((size_t)b * 4 + c) * p.HW + hw];
      }
    }
    float x0pp[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SOLVER == kSolverDpmpp3M) {
      if (k.c_2 != 0.f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) x0pp[c] = p.hist2[((size_t)b * 4 + c) * p.HW + hw];
      }
      if (k.c_1 != 0.f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) x0p[c] = p.hist[((size_t)b * 4 + c) * p.HW + hw];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float ec = ld_f(p.eps, ((size_t)b * p.HW + hw) * p.eps_ld + c, p.eps_dt);
      float e = ec;
      if (active) {
        const float eu = ld_f(p.eps, ((size_t)(p.n + b) * p.HW + hw) * p.eps_ld + c, p.eps_dt);
        e = __builtin_fmaf(ec - eu, sb, eu);
        if (p.factors) e = e * fb;
      }
      float x0;
      if constexpr (PRED == kPredictionV) {      // e holds v up to here
        const float v = e;
        x0 = __builtin_fmaf(x[c], k.sqrt_a, -(v * k.sqrt_1ma));
        if constexpr (SOLVER == kSolverDdim) e = __builtin_fmaf(v, k.sqrt_a, x[c] * k.sqrt_1ma);
      } else {
        x0 = __builtin_fmaf(-e, k.sqrt_1ma, x[c]) / k.sqrt_a;
      }
      if constexpr (SOLVER == kSolverDpmpp2M) {
        p.hist[((size_t)b * 4 + c) * p.HW + hw] = x0;
        float acc = k.c_1 * x0p[c];
        acc = __builtin_fmaf(x0, k.c_0, acc);
        x[c] = __builtin_fmaf(x[c], k.c_x, acc);
      } else if constexpr (SOLVER == kSolverDpmpp3M) {
        float acc = k.c_2 * x0pp[c];
        acc = __builtin_fmaf(x0p[c], k.c_1, acc);
        acc = __builtin_fmaf(x0, k.c_0, acc);
        x[c] = __builtin_fmaf(x[c], k.c_x, acc);
        if (k.c_1 != 0.f) p.hist2[((size_t)b * 4 + c) * p.HW + hw] = x0p[c];
        p.hist[((size_t)b * 4 + c) * p.HW + hw] = x0;
      } else if constexpr (SOLVER == kSolverRow1) {
        const float acc = x0 * k.c_0;
        x[c] = __builtin_fmaf(x[c], k.c_x, acc);
      } else {
        const float en = e * k.sqrt_1map;
        x[c] = c < 2 ? x0 * k.sqrt_ap + en : __builtin_fmaf(x0, k.sqrt_ap, en);
      }
    }
    if constexpr (SEEDED) {
      const float cz = SOLVER == kSolverDdim ? k.sigma : k.c_z;
      if (cz != 0.f) {
        float z[4];
        seeded_normal4(p.seeds.v[b], (uint32_t)hw, draw_sigma((uint32_t)idx), z);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = __builtin_fmaf(z[c], cz, x[c]);
      }
    }
  }
  if (p.mask && next < p.n_steps_total) {
    const StepCoef kn = p.table[next];
    float z[4];
    if constexpr (SEEDED) seeded_normal4(p.seeds.v[b], (uint32_t)hw, draw_blend((uint32_t)next), z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t e = ((size_t)b * 4 + c) * p.HW + hw;
      if (!p.mask[e]) {
        float zn;
        if constexpr (SEEDED) zn = z[c]; else zn = p.step_noise[(size_t)next * p.n * 4 * p.HW + e];
        x[c] = p.ref[e] * kn.sqrt_a + zn * kn.sqrt_1ma;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) p.latent[((size_t)b * 4 + c) * p.HW + hw] = x[c];
  for (int r = 0; r < p.in_rep; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) st_f(p.unet_in, ((size_t)(r * p.n + b) * p.HW + hw) * p.in_ld + c, p.in_dt, x[c]);
}
__global__ void ddim_advance_kernel(const StepCoef* table, int* step_idx, float* t_out, int do_update) {
  const int next = do_update ? *step_idx + 1 : 0;
  *step_idx = next;
  *t_out = table[next].t;     // table carries one sentinel entry past the last step
}
template <int PRED>
static void launch_step_pred(const StepParams& p, int do_update, dim3 grid, dim3 block, hipStream_t s) {
  if (p.solver == kSolverDpmpp2M) {
    if (p.seeded) hipLaunchKernelGGL((step_kernel<kSolverDpmpp2M, true, PRED>), grid, block, 0, s, p, do_update);
    else hipLaunchKernelGGL((step_kernel<kSolverDpmpp2M, false, PRED>), grid, block, 0, s, p, do_update);
  } else if (p.solver == kSolverRow1) {
    if (p.seeded) hipLaunchKernelGGL((step_kernel<kSolverRow1, true, PRED>), grid, block, 0, s, p, do_update);
    else hipLaunchKernelGGL((step_kernel<kSolverRow1, false, PRED>), grid, block, 0, s, p, do_update);
  } else if (p.solver == kSolverDpmpp3M) {
    if (p.seeded) hipLaunchKernelGGL((step_kernel<kSolverDpmpp3M, true, PRED>), grid, block, 0, s, p, do_update);
    else hipLaunchKernelGGL((step_kernel<kSolverDpmpp3M, false, PRED>), grid, block, 0, s, p, do_update);
  } else {
    if (p.seeded) hipLaunchKernelGGL((step_kernel<kSolverDdim, true, PRED>), grid, block, 0, s, p, do_update);
    else hipLaunchKernelGGL((step_kernel<kSolverDdim, false, PRED>), grid, block, 0, s, p, do_update);
  }
}
void launch_step(const StepParams& p, int do_update, hipStream_t s) {
  const size_t total = (size_t)p.n * p.HW;
  const dim3 grid((total + 255) / 256), block(256);
  if (p.prediction == kPredictionV) launch_step_pred<kPredictionV>(p, do_update, grid, block, s);
  else launch_step_pred<kPredictionEpsilon>(p, do_update, grid, block, s);
  hipLaunchKernelGGL(ddim_advance_kernel, dim3(1), dim3(1), 0, s, p.table, p.step_idx, p.t_out, do_update);
}

// ---------------------------------------------------------------------------------------------------------
// CFG rescale factors (kernels.h launch_cfg_rescale_factors): what the sampler runs in front of the per-step kernel where rescale is on.
// Chan merge of (nb, mb, M2b) into (na, ma, M2a), as in norm.hip
__device__ __forceinline__ void moments_merge(float& na, float& ma, float& m2a, float nb, float mb, float m2b) {
  if (nb == 0.f) return;
  const float n = na + nb;
  const float d = mb - ma;
  const float f = nb / n;
  ma = ma + d * f;
  m2a = m2a + m2b + d * d * na * f;
  na = n;
}
// One thread per latent pixel, grid (ceil(HW / 256), n): blockIdx.y is the entry, so the partition of an entry's pixels depends on HW alone.
// Each thread turns its four channel values of ec and of ecfg = fma(ec - eu, s_b, eu) into (4, mean, M2); lanes merge downwards
// (lane l takes lane l + o, o = 32 .. 1), wave 0..3 in order through LDS, and thread 0 leaves the block's two triples at
// partials[(b * blocks + block) * 6 ..].  Values are taken relative to the entry's pixel 0, channel 0 (M2 does not move under a shift, and
// every difference is then of the size of the spread, not of the mean): the means of the triples are relative to that pivot.
__global__ __launch_bounds__(kCfgMomentsBlock) void cfg_moments_kernel(const void* eps, int eps_dt, int eps_ld, int n, int HW,
                                                                       CfgScales scales, float* partials) {
#pragma clang fp contract(off)
  __shared__ float wave_part[kCfgMomentsBlock / 64][6];
  const int b = blockIdx.y;
  const int hw = blockIdx.x * kCfgMomentsBlock + threadIdx.x;
  const float sb = scales.v[b];
  const float pivot_c = ld_f(eps, (size_t)b * HW * eps_ld, eps_dt);
  const float pivot_u = ld_f(eps, (size_t)(n + b) * HW * eps_ld, eps_dt);
  const float pivot_g = __builtin_fmaf(pivot_c - pivot_u, sb, pivot_u);
  float cnt = 0.f, mc = 0.f, qc = 0.f, mg = 0.f, qg = 0.f;
  if (hw < HW) {
    float dc[4], dg[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float ec = ld_f(eps, ((size_t)b * HW + hw) * eps_ld + c, eps_dt);
      const float eu = ld_f(eps, ((size_t)(n + b) * HW + hw) * eps_ld + c, eps_dt);
      dc[c] = ec - pivot_c;
      dg[c] = __builtin_fmaf(ec - eu, sb, eu) - pivot_g;
    }
    cnt = 4.f;
    mc = ((dc[0] + dc[1]) + (dc[2] + dc[3])) * 0.25f;
    mg = ((dg[0] + dg[1]) + (dg[2] + dg[3])) * 0.25f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      qc = __builtin_fmaf(dc[c] - mc, dc[c] - mc, qc);
      qg = __builtin_fmaf(dg[c] - mg, dg[c] - mg, qg);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float nb = __shfl_down(cnt, o), mcb = __shfl_down(mc, o), qcb = __shfl_down(qc, o), mgb = __shfl_down(mg, o), qgb = __shfl_down(qg, o);
    float ng = cnt;
    moments_merge(cnt, mc, qc, nb, mcb, qcb);
    moments_merge(ng, mg, qg, nb, mgb, qgb);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wave_part[wave][0] = cnt; wave_part[wave][1] = mc; wave_part[wave][2] = qc;
    wave_part[wave][3] = cnt; wave_part[wave][4] = mg; wave_part[wave][5] = qg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ng = cnt;
    for (int w = 1; w < kCfgMomentsBlock / 64; ++w) {
      moments_merge(cnt, mc, qc, wave_part[w][0], wave_part[w][1], wave_part[w][2]);
      moments_merge(ng, mg, qg, wave_part[w][3], wave_part[w][4], wave_part[w][5]);
    }
    float* out = partials + ((size_t)b * gridDim.x + blockIdx.x) * 6;
    out[0] = cnt; out[1] = mc; out[2] = qc; out[3] = ng; out[4] = mg; out[5] = qg;
  }
}
// One wavefront per entry: 64 partials at a time are loaded one per lane, then merged in block-index order (every lane runs the same merge on
// the broadcast values, so the chain is arithmetic, not loads).  f_b = fma(phi, sqrt(M2c / M2g), 1 - phi); M2g == 0 gives 1.
__global__ __launch_bounds__(64) void cfg_factor_kernel(const float* partials, int blocks, float phi, float* factors) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* part = partials + (size_t)b * blocks * 6;
  float nc = 0.f, mc = 0.f, qc = 0.f, ng = 0.f, mg = 0.f, qg = 0.f;
  for (int base = 0; base < blocks; base += 64) {
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (base + lane < blocks) {
#pragma unroll
      for (int j = 0; j < 6; ++j) v[j] = part[(size_t)(base + lane) * 6 + j];
    }
    const int m = min(64, blocks - base);
    for (int j = 0; j < m; ++j) {
      moments_merge(nc, mc, qc, __shfl(v[0], j), __shfl(v[1], j), __shfl(v[2], j));
      moments_merge(ng, mg, qg, __shfl(v[3], j), __shfl(v[4], j), __shfl(v[5], j));
    }
  }
  if (lane == 0) factors[b] = qg == 0.f ? 1.f : __builtin_fmaf(phi, sqrtf(qc / qg), 1.f - phi);
}
void launch_cfg_rescale_factors(const void* eps, int eps_dt, int eps_ld, int n, int HW, const CfgScales& scales, float phi, float* partials,
                                float* factors, hipStream_t s) {
  const int blocks = cfg_moments_blocks(HW);
  hipLaunchKernelGGL(cfg_moments_kernel, dim3(blocks, n), dim3(kCfgMomentsBlock), 0, s, eps, eps_dt, eps_ld, n, HW, scales, partials);
  hipLaunchKernelGGL(cfg_factor_kernel, dim3(n), dim3(64), 0, s, (const float*)partials, blocks, phi, factors);
}
__global__ void axpby_kernel(float* dst, const float* a, float sa, const float* b, float sb, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = a[i] * sa + b[i] * sb;
}
void launch_axpby(float* dst, const float* a, float sa, const float* b, float sb, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(axpby_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, a, sa, b, sb, n);
}

// ---------------------------------------------------------------------------------------------------------
// ControlNet skip residuals: every segment of the table in one launch (kernels.h SkipSeg).  HBM-bound: one 16-byte chunk per lane and trip (8 halfs /
// 4 floats), consecutive lanes on consecutive chunks of the flattened segment list, a grid capped at 2048 workgroups striding over the rest.  A lane's
// chunk index only grows, so it walks the table forwards (a handful of uniform loads per segment change).  TABLE == false is the one-scalar form
// (K == 1, the scale is *scales, the plain fma at every scale); TABLE == true reads the K x 8 scales of the table row [*step_idx][K][8].
//  * Divisions are 32-bit: skip_table_check keeps a segment under 2^32 chunks, so chunk -> (row, chunk of the row) -> batch entry never takes the
//    64-bit division, which is a long instruction sequence here.
//  * The scales of the row sit in registers (32 at K = 4) and a chunk's are picked by compares, k and j unrolled: a dynamic index into a register
//    array would go through scratch.  A 16-byte chunk lies in one row and a row in one entry (C % 8 == 0, rows % B == 0).
//  * TABLE: a source at scale 0 is not read, and a chunk whose scales are all 0 is not written.  fma(0, r, dst) is NaN for a non-finite r, and the
//    sources of an iteration without a control forward are whatever the last one -- or nobody -- left there; a net that ran on the conditional
//    entries alone has a source that ends before the segment does.
//  * The sum stays in fp32 across the sources, one fma per live source in the order k = 0 .. K-1, and is rounded to T once: K nets cost a channel
//    one rounding, as one net does.
template <typename T, int K, bool TABLE>
__global__ __launch_bounds__(256) void skip_add_kernel(const SkipSeg* __restrict__ table, int n_seg, unsigned long long total,
                                                       const float* __restrict__ scales, const int* __restrict__ step_idx, unsigned B) {
  static_assert(TABLE || K == 1, "one scalar scales one source");
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int NS = TABLE ? kSkipScaleEntries : 1;
  typedef T vec_t __attribute__((ext_vector_type(E)));
  float sv[K][NS];
  {
    const float* row = scales;
    if constexpr (TABLE) row += (size_t)*step_idx * (K * NS);
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < NS; ++j) sv[k][j] = row[k * NS + j];
  }
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  int si = 0;
  SkipSeg g = table[0];
  unsigned long long end = n_seg > 1 ? table[1].first : total;
  unsigned rpe = 1;      // rows per batch entry
  if constexpr (TABLE) rpe = (unsigned)g.rows / B;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    while (i >= end) {      // (i < total = the last segment's end: si stays inside the table)
      ++si;
      g = table[si];
      end = si + 1 < n_seg ? table[si + 1].first : total;
      if constexpr (TABLE) rpe = (unsigned)g.rows / B;
    }
    const unsigned l = (unsigned)(i - g.first);
    const unsigned cpr = (unsigned)g.C / E;
    const unsigned row = l / cpr;
    const unsigned cc = l - row * cpr;
    float sc[K];
    if constexpr (TABLE) {
      const unsigned b = row / rpe;      // (a segment that holds a chunk has rows >= B: rpe >= 1, and b < B)
      bool any = false;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        sc[k] = sv[k][0];
#pragma unroll
        for (int j = 1; j < NS; ++j) sc[k] = b == (unsigned)j ? sv[k][j] : sc[k];
        any = any || sc[k] != 0.f;
      }
      if (!any) continue;
    } else {
      sc[0] = sv[0][0];
    }
    vec_t* d = reinterpret_cast<vec_t*>(reinterpret_cast<T*>(g.dst) + (unsigned long long)row * (unsigned long long)g.dst_ld) + cc;
    vec_t v = *d;
    float f[E];
#pragma unroll
    for (int j = 0; j < E; ++j) f[j] = (float)v[j];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (TABLE && sc[k] == 0.f) continue;
      const vec_t a = reinterpret_cast<const vec_t*>(g.src[k])[l];
#pragma unroll
      for (int j = 0; j < E; ++j) f[j] = fmaf(sc[k], (float)a[j], f[j]);
    }
#pragma unroll
    for (int j = 0; j < E; ++j) v[j] = (T)f[j];
    *d = v;
  }
}
// SiLU in place over a dense tensor (a control net's hint embedder, once per hint: off the per-step path and left plain)
__global__ void silu_inplace_kernel(void* p, int dt, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st_f(p, i, dt, silu_f(ld_f(p, i, dt)));
}
void launch_silu_inplace(void* p, int dt, size_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(silu_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, dt, n);
}
const char* skip_table_check(SkipSeg* t, int n_seg, int K, int B, int dt, unsigned long long* total_chunks) {
  if (dt != DT_F32 && dt != DT_F16) return "skip residual add: the dtype must be fp32 or f16 (the stream dtype of the UNet)";
  if (n_seg < 1 || !t) return "skip residual add: at least one segment";
  if (K < 1 || K > kSkipMaxSources) return "skip residual add: the number of sources K must be in 1..4";
  if (B < 0 || B > kSkipScaleEntries) return "skip residual add: B must be in 1..8";
  const size_t es = dt_size(dt);
  unsigned long long total = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (t[i].rows < 0 || t[i].C <= 0) return "skip residual add: rows must be >= 0 and C > 0";
    if (t[i].C % 8 != 0) return "skip residual add: C must be a multiple of 8";
    if (t[i].dst_ld < t[i].C) return "skip residual add: dst_ld must be >= C";
    uintptr_t bits = (uintptr_t)t[i].dst | (uintptr_t)((size_t)t[i].dst_ld * es);
    bool null = !t[i].dst;
    for (int k = 0; k < K; ++k) { null = null || !t[i].src[k]; bits |= (uintptr_t)t[i].src[k]; }
    if (null) return "skip residual add: null segment pointer";
    if (bits & 15) return "skip residual add: dst, src and the row pitch of dst must be 16-byte aligned";
    const unsigned long long chunks = (unsigned long long)t[i].rows * (unsigned long long)((size_t)t[i].C * es / 16);
    if (chunks >> 32) return "skip residual add: a segment must be smaller than 2^32 16-byte chunks";
    if (B && t[i].rows % B != 0) return "skip residual add: every segment's rows must be a multiple of B (equal rows per batch entry)";
    t[i].first = total;
    total += chunks;
  }
  if (total_chunks) *total_chunks = total;
  return nullptr;
}
using SkipAddKernel = void (*)(const SkipSeg*, int, unsigned long long, const float*, const int*, unsigned);
template <typename T>      // [0]: one scalar; [K]: the table form with K sources
static constexpr SkipAddKernel kSkipAdd[1 + kSkipMaxSources] = {skip_add_kernel<T, 1, false>, skip_add_kernel<T, 1, true>, skip_add_kernel<T, 2, true>,
                                                                skip_add_kernel<T, 3, true>, skip_add_kernel<T, 4, true>};
void launch_skip_add(const SkipSeg* table_dev, int n_seg, int K, unsigned long long total_chunks, const float* scales_dev, const int* step_idx_dev, int B,
                     int dt, hipStream_t s) {
  if (!total_chunks) return;
  if (K < 1 || K > kSkipMaxSources || (!step_idx_dev && K != 1)) throw std::runtime_error("skip residual add: the number of sources K must be in 1..4, 1 under one scalar");      // (skip_table_check)
  const unsigned grid = (unsigned)std::min<unsigned long long>((total_chunks + 255) / 256, 2048);
  const int form = step_idx_dev ? K : 0;
  hipLaunchKernelGGL(dt == DT_F16 ? kSkipAdd<half_t>[form] : kSkipAdd<float>[form], dim3(grid), dim3(256), 0, s, table_dev, n_seg, total_chunks, scales_dev,
                     step_idx_dev, (unsigned)B);
}

// ---------------------------------------------------------------------------------------------------------
// image post-process, stablediffusion/mod.rs:210-230: ((x+1)/2)*255 -> clamp [0,255] -> truncating u8 cast
__global__ void to_u8_kernel(const void* src, int dt, int lds_, unsigned char* dst, size_t pixels) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pixels * 3) return;
  const size_t pix = i / 3;
  const int c = i - pix * 3;
  float v = ld_f(src, pix * lds_ + c, dt);
  v = ((v + 1.0f) / 2.0f) * 255.0f;
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  dst[i] = (unsigned char)v;
}
void launch_to_u8_image(const void* src, int dt, int lds_, unsigned char* dst, size_t pixels, hipStream_t s) {
  hipLaunchKernelGGL(to_u8_kernel, dim3((pixels * 3 + 255) / 256), dim3(256), 0, s, src, dt, lds_, dst, pixels);
}
// image_to_latent pre-processing :239-255: (u8/255)*2 - 1
__global__ void from_u8_kernel(const unsigned char* src, void* dst, int dt, int ldd, size_t pixels) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pixels * 3) return;
  const size_t pix = i / 3;
  const int c = i - pix * 3;
  st_f(dst, pix * ldd + c, dt, ((float)src[i] / 255.0f) * 2.0f - 1.0f);
}
void launch_from_u8_image(const unsigned char* src, void* dst, int dt, int ldd, size_t pixels, hipStream_t s) {
  hipLaunchKernelGGL(from_u8_kernel, dim3((pixels * 3 + 255) / 256), dim3(256), 0, s, src, dst, dt, ldd, pixels);
}

// ---------------------------------------------------------------------------------------------------------
// synthetic weights: bit-identical to oracle/config.py::synth_values (integer hash, one fp32 mul, one fp32 add)
__global__ void synth_fill_kernel(float* dst, size_t numel, uint64_t key, float scale, float mean) {
#pragma clang fp contract(off)   // numpy rounds the product and the sum separately; an FMA here would differ by 1 ulp
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numel) return;
  uint64_t z = key + (uint64_t)i * 0xD1342543DE82EF95ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const float u = (float)(uint32_t)(z >> 40) * 5.9604644775390625e-08f;   // * 2^-24, exact
  const float t = u - 0.5f;                                                // exact
  const float prod = t * scale;
  dst[i] = prod + mean;
}
void launch_synth_fill(float* dst, size_t numel, uint64_t key, float scale, float mean, hipStream_t s) {
  hipLaunchKernelGGL(synth_fill_kernel, dim3((numel + 255) / 256), dim3(256), 0, s, dst, numel, key, scale, mean);
}

__device__ __forceinline__ int geglu_unpermute(int pcol, int N) {
  // packed column -> original column: 32-wide groups = 16 x columns then their 16 gate columns
  const int g = pcol >> 5, w = pcol & 31, nh = N >> 1;
  return w < 16 ? g * 16 + w : nh + g * 16 + (w - 16);
}
// max |x| of a tensor (power-of-two weight scale of the split-operand packing): one atomicMax on the float bits per block
__global__ void absmax_kernel(const float* src, size_t n, unsigned* out) {
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(src[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));      // non-negative floats order like their bit patterns
}
void launch_absmax(const float* src, size_t n, float* out_dev, hipStream_t s, bool accumulate) {
  if (!accumulate) (void)hipMemsetAsync(out_dev, 0, sizeof(float), s);
  const unsigned blocks = (unsigned)std::min<size_t>(1024, (n + 255) / 256);
  hipLaunchKernelGGL(absmax_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, src, n, reinterpret_cast<unsigned*>(out_dev));
}
__global__ void pack_linear_kernel(const float* src, void* dst, int dt, int K, int N, int Kpad, int Npad, int geglu,
                                   int n_offset, const float* kscale, float wscale) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)Npad * Kpad) return;
  const int np = i / Kpad;
  const int k = i - (size_t)np * Kpad;
  float v = 0.f;
  if (np < N && k < K) {
    const int n = geglu ? geglu_unpermute(np, N) : np;
    v = src[(size_t)k * N + n];
    if (kscale) v *= kscale[k];       // LayerNorm gamma folded into the projection (W' = diag(gamma) W)
    v *= wscale;                      // power of two (DT_HL packing), 1 otherwise
  }
  st_f(dst, ((size_t)n_offset + np) * Kpad + k, dt, v);
}
void launch_pack_linear(const float* src, void* dst, int dt, int K, int N, int Kpad, int Npad, int geglu, int n_offset,
                        hipStream_t s, const float* kscale, float wscale) {
  const size_t total = (size_t)Npad * Kpad;
  hipLaunchKernelGGL(pack_linear_kernel, dim3((total + 255) / 256), dim3(256), 0, s, src, dst, dt, K, N, Kpad, Npad, geglu, n_offset,
                     kscale, wscale);
}
__global__ void pack_linear_hilo_kernel(const float* src, half_t* dst, int K, int N, int Npad, int geglu, float lo_scale, int mode, int n_offset) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)Npad * 2 * K) return;
  const int np = (int)(i / (2 * (size_t)K));
  const int k2 = (int)(i - (size_t)np * 2 * K);
  int part = k2 >= K ? 1 : 0, k = k2 - part * K;
  if (mode == 2) { part = 0; k = 16 * (k2 >> 5) + (k2 & 15); }       // HL16 interleave: both copies of a 16-channel group carry the weight itself
  half_t v = (half_t)0.f;
  if (np < N) {
    const int n = geglu ? geglu_unpermute(np, N) : np;
    float w = src[(size_t)k * N + n];
    asm("" : "+v"(w));
    const half_t hi = (half_t)w;
    v = !part ? hi : mode == 0 ? (half_t)((w - (float)hi) * lo_scale) : (half_t)((float)hi / lo_scale);
  }
  dst[i + (size_t)n_offset * 2 * K] = v;
}
void launch_pack_linear_hilo(const float* src, void* dst, int K, int N, int Npad, int geglu, float lo_scale, hipStream_t s, int mode, int n_offset) {
  const size_t total = (size_t)Npad * 2 * K;
  hipLaunchKernelGGL(pack_linear_hilo_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, reinterpret_cast<half_t*>(dst), K, N, Npad, geglu, lo_scale, mode, n_offset);
}
// cs[r] = sum_k packed[r][k] over the ROUNDED packed values (what the MFMA really multiplies), one wave per packed row
// kscale (K values, optional): cs[r] = sum_k kscale[k] * packed[r][k] -- the shadow form of a folded LayerNorm, whose gamma rides on the A operand
__global__ void colsum_packed_kernel(const void* wp, int dt, int Kpad, int nrows, float* cs, const float* kscale, int K, int interleave) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nrows) return;
  float acc = 0.f;
  if (kscale && interleave) {      // K weights twice in the HL16 interleave: k sits at 32 (k >> 4) + (k & 15)
    for (int k = lane; k < K; k += 64) acc = fmaf(kscale[k], ld_f(wp, (size_t)row * Kpad + 32 * (k >> 4) + (k & 15), dt), acc);
  } else
  if (kscale) { for (int k = lane; k < K; k += 64) acc = fmaf(kscale[k], ld_f(wp, (size_t)row * Kpad + k, dt), acc); }
  else for (int k = lane; k < Kpad; k += 64) acc += ld_f(wp, (size_t)row * Kpad + k, dt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) cs[row] = acc;
}
void launch_colsum_packed(const void* wp, int dt, int Kpad, int nrows, float* cs, hipStream_t s, const float* kscale, int K, int interleave) {
  hipLaunchKernelGGL(colsum_packed_kernel, dim3((nrows + 3) / 4), dim3(256), 0, s, wp, dt, Kpad, nrows, cs, kscale, K, interleave);
}
// out[n] = sum_k beta[k] * W[k][n] + bias[n]   (canonical column order; W is the burn [K][N] layout)
__global__ void beta_dot_kernel(const float* w, const float* beta, const float* bias, float* out, int K, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float acc = bias ? bias[n] : 0.f;
  for (int k = 0; k < K; ++k) acc += beta[k] * w[(size_t)k * N + n];
  out[n] = acc;
}
void launch_beta_dot(const float* w, const float* beta, const float* bias, float* out, int K, int N, hipStream_t s) {
  hipLaunchKernelGGL(beta_dot_kernel, dim3((N + 255) / 256), dim3(256), 0, s, w, beta, bias, out, K, N);
}
__global__ void pack_conv_kernel(const float* src, void* dst, int dt, int Cout, int Cin, int ks, int Kpad, int Npad, float wscale) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)Npad * Kpad) return;
  const int n = i / Kpad;
  const int k = i - (size_t)n * Kpad;
  float v = 0.f;
  if (n < Cout && k < ks * ks * Cin) {
    const int tap = k / Cin, c = k - tap * Cin;
    const int ky = tap / ks, kx = tap - ky * ks;
    v = src[(((size_t)n * Cin + c) * ks + ky) * ks + kx] * wscale;     // wscale: power of two (DT_HL packing), 1 otherwise
  }
  st_f(dst, i, dt, v);
}
void launch_pack_conv(const float* src, void* dst, int dt, int Cout, int Cin, int ks, int Kpad, int Npad, hipStream_t s, float wscale) {
  const size_t total = (size_t)Npad * Kpad;
  hipLaunchKernelGGL(pack_conv_kernel, dim3((total + 255) / 256), dim3(256), 0, s, src, dst, dt, Cout, Cin, ks, Kpad, Npad, wscale);
}
// canonical 3x3 conv [Cout][Cin][3][3] -> the four 2x2 phase convolutions of "nearest-2x upsample, then that conv" [4][Cout][Cin][2][2] (upsample_fold.h)
__global__ void fold_upsample_kernel(const float* src, float* dst, size_t pairs) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < 16 * pairs) dst[e] = fold_element(src, pairs, e);
}
void launch_fold_upsample(const float* src, float* dst, int Cout, int Cin, hipStream_t s) {
  const size_t pairs = (size_t)Cout * Cin;
  hipLaunchKernelGGL(fold_upsample_kernel, dim3((unsigned)((16 * pairs + 255) / 256)), dim3(256), 0, s, src, dst, pairs);
}
__global__ void pack_bias_kernel(const float* src, float* dst, int N, int Npad, int geglu, int n_offset) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Npad) return;
  float v = 0.f;
  if (i < N && src) v = src[geglu ? geglu_unpermute(i, N) : i];
  dst[n_offset + i] = v;
}
void launch_pack_bias(const float* src, float* dst, int N, int Npad, int geglu, int n_offset, hipStream_t s) {
  hipLaunchKernelGGL(pack_bias_kernel, dim3((Npad + 255) / 256), dim3(256), 0, s, src, dst, N, Npad, geglu, n_offset);
}

}  // namespace sdxl
