// Fast-path implicit GEMM for gfx950: f16 operands, direct-to-LDS staging through an NS-deep ring.  PRODUCTION kernels only:
// the A/B partners, rolled loops, measurement modes and the loader-wave experiment live in igemm_measure.hip (measure builds).
//
// Same contract as igemm_kernel (igemm.hip) for the shapes that dominate the SDXL step (f16 activations, Cin % 64 == 0,
// 16-byte aligned rows); everything else stays on the generic kernel.  What every kernel in this file shares (CDNA4-specific):
//   * HBM/L2 -> LDS without a VGPR round trip: every wave issues `global_load_lds_dwordx4` (16 B per lane, 1 KiB per wave
//     instruction = 8 tile rows of 128 B).  The LDS image is lane-linear, so the bank-conflict swizzle is applied to the
//     per-lane SOURCE address (chunk ^ f(row)) and again on the fragment read; halo / tail rows fetch from a zero page.
//     The conv gather (tap, stride, fused nearest-2x upsample) is still just a per-lane source address.
//   * NS-deep LDS ring with COUNTED `s_waitcnt vmcnt(N)` across a raw s_barrier; one barrier per k-tile.
//   * v_mfma_f32_32x32x16_f16 with the operand roles swapped (weights = MFMA A operand, activations = B operand): the
//     accumulator layout then gives each lane 4 CONSECUTIVE output columns of one row, and GEGLU pairs (x, gate) sit in the
//     same lane of the same accumulator tile.
//   * swizzle f(row) = (row>>1)&7 makes the ds_read_b128 fragment reads of 32 rows conflict-free across the four 16-lane
//     service groups (two 128-byte tile rows share one 256-byte bank row); measured SQ_LDS_BANK_CONFLICT = 0.
//   * XCD-aware block -> tile mapping; epilogue staged through LDS so loads/stores are whole row segments; folded LayerNorm
//     (igemm_common.h).
// Kernels, in file order (selection: launch_igemm_glds at the bottom; measurements: DESIGN.md section 3.1):
//   igemm_glds_kernel  4 waves, 2-slot ring, several co-resident blocks per CU           (forced fallback variants 4 / 6)
//   igemm_pipe_kernel  6 / 8 waves, hand-ordered k-loop unrolled by the ring depth: counted lgkmcnt / vmcnt, register-double-
//                      buffered fragments, DMA pieces between the MFMAs; tiles 256x128, 128x128, 96x128, 256x160, 128x160;
//                      f16, strict f32 (4 x v_mfma_f32_32x32x2_f32) and the fused cross-attention instantiations
//   igemm_wide_kernel  256x320 tile, k-tile 32                                           (GEGLU projections)
#include "igemm_common.h"
#include <atomic>

namespace sdxl {

template <int BM, int BN, int NS, int MINB = 2>
__global__ __launch_bounds__(256, MINB) void igemm_glds_kernel(const IgemmParams p, const void* zeros) {
  kernarg_prefetch<(int)sizeof(IgemmParams) + 8>();   // every argument line in flight at once (one wait instead of five)   // >= MINB blocks per CU
  constexpr int WM = BM / 2, WN = BN / 2;     // wave tile
  constexpr int TM = WM / 32, TN = WN / 32;   // 32x32 MFMA tiles per wave
  constexpr int AJ = BM / 32, BJ = BN / 32;   // DMA instructions per wave per k-tile (8 rows each, 4 waves)
  constexpr int PER = AJ + BJ;                // DMA instructions per wave per stage
  constexpr int KT = 64;                      // f16 elements per k-tile = one 128-byte row
  constexpr int STAGE = (BM + BN) * 128;      // bytes per ring slot: A tile then B tile
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  const int tilesN = (p.N + BN - 1) / BN;
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  // Each XCD (private 4 MiB L2) owns a contiguous run of remapped ids.  Walk that run so the LARGER operand is read from
  // HBM by one XCD only: weights bigger than activations (the M=2048 transformer GEMMs) -> an XCD owns a range of weight
  // column tiles and sweeps all row tiles; otherwise (convs at 64^2/128^2, VAE) it owns row tiles and sweeps the weights.
  const int tilesM = (p.M + BM - 1) / BM;
  int tm, tn;
  if ((size_t)p.N * p.K > (size_t)p.M * p.Cin) { tn = bid / tilesM; tm = bid - tn * tilesM; }
  else { tm = bid / tilesN; tn = bid - tm * tilesN; }
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- DMA geometry: instruction j of this wave covers tile rows (j*4 + wave)*8 .. +7; lane -> (row, slot)
  const int lrow = lane >> 3, slot = lane & 7;
  const int HWo = p.Hout * p.Wout;
  const int Hup = p.Hin << p.up, Wup = p.Win << p.up;
  int rb[AJ], ry[AJ], rx[AJ], rsw[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int row = (j * 4 + wave) * 8 + lrow;
    const int m = m0 + row;
    rsw[j] = (slot ^ ((row >> 1) & 7)) * 8;       // source chunk (elements) that lands in this lane's LDS slot
    if (m < p.M) {
      const int b = m / HWo;
      const int rem = m - b * HWo;
      const int oy = rem / p.Wout;
      rb[j] = b; ry[j] = oy * p.stride - p.pad; rx[j] = (rem - oy * p.Wout) * p.stride - p.pad;
    } else { rb[j] = -1; ry[j] = -(1 << 28); rx[j] = 0; }
  }
  const half_t* Ag = reinterpret_cast<const half_t*>(p.A);
  // Incremental DMA source pointers: stage() is called for k-tiles 0,1,2,... in order, so the per-lane source address of
  // every tile row is a running pointer that advances by 64 elements per k-tile and is recomputed (bounds test, pixel
  // address) only when the k-tile crosses into the next filter tap -- no per-tile integer division or 64-bit multiply.
  const half_t* wptr[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int row = (j * 4 + wave) * 8 + lrow;
    wptr[j] = reinterpret_cast<const half_t*>(p.W) + (size_t)(n0 + row) * p.Kpad + (slot ^ ((row >> 1) & 7)) * 8;
  }
  const half_t* aptr[AJ];
  int aadv[AJ];
  int s_c0 = 0, s_dy = 0, s_dx = 0;      // wave-uniform tap walk state
  auto retap = [&]() {
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int iy = ry[j] + s_dy, ix = rx[j] + s_dx;
      const bool ok = (unsigned)iy < (unsigned)Hup && (unsigned)ix < (unsigned)Wup;   // rows beyond M carry iy << 0
      const size_t off = (((size_t)(rb[j] < 0 ? 0 : rb[j]) * p.Hin + ((ok ? iy : 0) >> p.up)) * p.Win + ((ok ? ix : 0) >> p.up)) * p.lda + rsw[j];
      aptr[j] = ok ? Ag + off : reinterpret_cast<const half_t*>(zeros);
      aadv[j] = ok ? KT : 0;
    }
  };
  retap();

  auto stage = [&](int buf) {
    char* la = smem + buf * STAGE + wave * 1024;
    char* lb = la + BM * 128;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      __builtin_amdgcn_global_load_lds((gptr_t)aptr[j], (lptr_t)(la + j * 4096), 16, 0, 0);
      aptr[j] += aadv[j];
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      __builtin_amdgcn_global_load_lds((gptr_t)wptr[j], (lptr_t)(lb + j * 4096), 16, 0, 0);
      wptr[j] += KT;
    }
    s_c0 += KT;
    if (s_c0 == p.Cin) {                 // next k-tile starts a new tap (uniform branch)
      s_c0 = 0;
      if (++s_dx == p.ksize) { s_dx = 0; ++s_dy; }
      retap();
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = p.Kpad / KT;
  const int fr = lane & 31, fh = lane >> 5;
  // prologue: NS-1 tiles in flight
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) stage(s);
  float lnA[TM], lnC[TM];
  ln_prologue<TM>(p, m0 + wm * WM, fr, lnA, lnC);
  int cur = 0;                 // ring slot of tile kt
  int nxt = NS - 1;            // ring slot tile kt+NS-1 goes to (= slot of tile kt-1)
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt must have landed; tiles kt+1 .. kt+NS-2 may stay in flight (only if they were really issued)
    if (kt + NS - 2 < nk) wait_vmcnt<PER * (NS - 2)>(); else wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();          // all waves: tile kt visible, compute(kt-1) finished -> slot `nxt` is free
    asm volatile("" ::: "memory");
    if (kt + NS - 1 < nk) stage(nxt);
    const char* a = smem + cur * STAGE;
    const char* b = a + BM * 128;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ch = kk * 2 + fh;
      half8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WM + i * 32 + fr;
        fa[i] = *reinterpret_cast<const half8*>(a + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * WN + j * 32 + fr;
        fb[j] = *reinterpret_cast<const half8*>(b + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)   // weights as the A operand (rows = n), activations as B (cols = m)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
    nxt = cur;
    cur = cur + 1 == NS ? 0 : cur + 1;
  }

  __syncthreads();                                 // every wave is done reading the ring: it becomes the staging area
  igemm_epilogue_staged<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, lane, smem + wave * (WM * WN * 4), lnA, lnC, zeros);
}

// ---------------------------------------------------------------------------------------------------------
// 8-wave software-pipelined kernel (one 512-thread workgroup per CU, two waves per SIMD).
//
// Why a second structure: in the 4-wave kernel above every kk-step is {4 ds_read_b128 -> lgkmcnt(0) -> 4 MFMA} on ONE
// fragment register set and every k-tile starts with vmcnt(0), so LDS latency and DMA latency are both exposed and the
// matrix pipe idles ~2/3 of the time (measured 25..35 % MFMA utilisation).  Here the k-loop is hand ordered:
//   * fragments are double buffered in registers: the ds_reads of step kk+1 are issued before the MFMAs of step kk and
//     waited for with a COUNTED lgkmcnt (hipcc only emits lgkmcnt(0) across the loop back edge, so the reads are inline
//     asm and every wait is followed by sched_barrier(0) so no MFMA is hoisted above it);
//   * the ring is NS >= 3 deep and the DMA wait is counted too: at the single barrier of k-tile kt (between its third and
//     fourth kk-step) a wave waits only for its own pieces of tile kt+1; the pieces of tile kt+NS-1 -- issued BETWEEN the
//     MFMAs of the first three steps, into the slot the previous barrier freed -- stay in flight across the raw s_barrier.
//     After the barrier the first fragments of tile kt+1 are prefetched under the fourth step;
//   * WGM = waves along M (4: 4x2 wave grid, 8: 8x1 -- the 256x160 tile, 3: the 6-wave 96x128 tile).  BN need not be a
//     multiple of 64: the weight tile's BN/8 eight-row pieces are dealt round-robin, waves below REM carry one more piece
//     and wait on their own count.
//   * S2 ("two k-tiles per rendezvous", rings of >= 4 slots): the vmcnt wait + s_barrier run in every SECOND k-tile only and cover the
//     next TWO tiles; the DMA lead is one tile shorter (tile kt + NS - 2 goes into the slot of tile kt - 2, which the last barrier
//     -- in tile kt - 1 or kt - 2 -- has freed).  Half the rendezvous of a launch for one tile less in flight.
// TSW ("transposed by operand swap", f16 256x128 only): workgroups whose whole tile lies in the transposed part of the output (the V^T
// columns of a fused QKV projection) run a copy of the k-loop with the MFMA operand roles swapped -- activations as the A operand -- so a
// lane's accumulators are 4 x 4 consecutive ROWS (keys) of one column: the transposed store is then the direct row-per-lane epilogue
// (permlane32 half swap, 16-byte stores along the key axis) instead of the LDS-staged transpose (12.6 k cycles per 64x64 wave tile, the
// longest epilogue of the launch: tools/timeline_probe.py).  Same products, same k order: bit-identical values.
// XH (with XA, round 6): the fused cross-attention at split precision (xattn_inplace_hl: hi / lo context images, three MFMAs per product)
template <int BM, int BN, int NS, int WGM = 4, int NW = 8, typename T = half_t, bool XA = false, bool S2 = false, bool TSW = false, bool XH = false>
__global__ __launch_bounds__(64 * NW) void igemm_pipe_kernel(const IgemmParams p, const void* zeros) {
  kernarg_prefetch<(int)sizeof(IgemmParams) + 8>();   // every argument line in flight at once (one wait instead of five)
  typedef typename PipeElem<T>::frag frag_t;
  constexpr int CE = 16 / (int)sizeof(T);     // elements per 16-byte chunk: 8 (f16) or 4 (f32, strict mode)
  constexpr int WGN = NW / WGM;               // NW waves per workgroup (8, or 4 with twice the wave tile)
  constexpr int WM = BM / WGM, WN = BN / WGN; // wave tile
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int NF = TM + TN;                 // ds_read_b128 per kk-step
  constexpr int BPC = BN / 8;                 // 8-row pieces of the weight tile
  constexpr int AJ = BM / (8 * NW), BJ = (BPC + NW - 1) / NW;   // DMA pieces per wave per k-tile (8 rows each, NW waves)
  constexpr int REM = BPC % NW;               // waves >= REM (when REM != 0) have no last weight piece
  constexpr int PER = AJ + BJ;
  static_assert(BM % (8 * NW) == 0 && WM % 32 == 0 && WN % 32 == 0 && BN % 8 == 0, "bad tile");
  constexpr int KT = 8 * CE;                  // elements per k-tile = one 128-byte row (64 f16 / 32 f32)
  constexpr int STAGE = (BM + BN) * 128;
  constexpr bool LIN = XA;                    // linear-only instantiation: scalar-base DMA addressing, no tap walk
  static_assert(NS >= 3, "counted-wait pipeline needs a ring of at least 3 slots");
  static_assert(BM * 128 + (TN - 1) * 4096 < 65536, "fragment offsets must fit the ds_read immediate");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const bool lastb = REM == 0 || wave < REM;  // this wave carries weight piece BJ-1

  const int tilesN = (p.N + BN - 1) / BN;
  const int tilesM = (p.M + BM - 1) / BM;
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  // split-K (grid = tiles x SK): consecutive remapped ids = the SK k-slices of one tile, so a tile's slices share an XCD
  // (its L2 then serves the partial slabs to the reducing workgroup at the same-XCD rate; placement is speed only)
  const int SK = p.splitk > 1 ? p.splitk : 1;
  const int slice = SK > 1 ? bid % SK : 0;
  if (SK > 1) bid /= SK;
  const int tile_id = bid;
  int tm, tn;
  if ((size_t)p.N * p.K > (size_t)p.M * p.Cin) { tn = bid / tilesM; tm = bid - tn * tilesM; }
  else { tm = bid / tilesN; tn = bid - tm * tilesN; }
  const int m0 = tm * BM, n0 = tn * BN;
  // phase form of an upsample convolution (IgemmParams::ph_rows; a row tile lies in one phase): this tile's phase 2a + b selects its weights and
  // the pad of each axis (tap (dy, dx) of row (i, j) reads source pixel (i + dy - pad + a, j + dx - pad + b)); mph = the phase's first row
  const int ph = p.ph_rows ? m0 / p.ph_rows : 0;
  const int mph = ph * p.ph_rows, pady = p.pad - (ph >> 1), padx = p.pad - (ph & 1);
  // TSW: the whole tile in the transposed part, whole 8-key pieces inside one batch entry, f16 out -> operand-swapped k-loop + direct transposed store
  bool tsw_swapped = false;
  if constexpr (TSW) {
    const int ok = n0 >= p.n_split && n0 + BN <= p.N && p.c_dt == DT_F16 && p.act == 0 && !p.epi_staged && (p.rpb % BM) == 0 && m0 + BM <= p.M &&
                   (p.ct_ld & 7) == 0 && (reinterpret_cast<uintptr_t>(p.Ct) & 15) == 0 && (!p.ln_stat || p.ln_slots <= 24);
    tsw_swapped = __builtin_amdgcn_readfirstlane(ok) != 0;
  }
  // counted DMA wait: K tiles of this wave's pieces may stay in flight
  auto wait_tiles = [&](auto KK) {
    constexpr int k = decltype(KK)::value;
    if constexpr (REM == 0) wait_vmcnt<PER * k>();
    else { if (lastb) wait_vmcnt<PER * k>(); else wait_vmcnt<(PER - 1) * k>(); }
  };

  // ---- DMA geometry: piece j of this wave covers tile rows (j*8 + wave)*8 .. +7; lane -> (row, slot)
  const int lrow = lane >> 3, slot = lane & 7;
  // weight rows first: they need no pixel arithmetic, and inside a UNet step the weights are the operand that arrives cold (the
  // activations were written by the previous launch) -- tile 0's weight pieces go out BEFORE the activation geometry below is
  // worked out (~1.5 k cycles earlier).  The in-order vmcnt accounting is unchanged: tile 0's pieces are still this wave's oldest.
  // Measured on the bench line, two libraries on one box: 23.30 / 23.27 -> 23.23 / 23.24 ms per step (profiles/r03_weights_first_ab.txt).
  const T* wptr[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int row = (j * NW + wave) * 8 + lrow;
    wptr[j] = reinterpret_cast<const T*>(reinterpret_cast<const char*>(p.W) + (size_t)ph * p.ph_wbytes) + (size_t)(n0 + row) * p.Kpad + (slot ^ ((row >> 1) & 7)) * CE;
  }
  // this workgroup's k-tiles [kbeg, kbeg + nk) of the Kpad / KT of the contraction (split-K: slice `slice` of SK)
  const int nk_all = p.Kpad / KT;
  const int kbeg = SK > 1 ? (int)((long)slice * nk_all / SK) : 0;
  const int nk = SK > 1 ? (int)((long)(slice + 1) * nk_all / SK) - kbeg : nk_all;
  if (kbeg > 0) {
#pragma unroll
    for (int j = 0; j < BJ; ++j) wptr[j] += kbeg * KT;
  }
  constexpr bool B0_EARLY = !LIN;      // (the scalar-base form of the fused cross-attention projections keeps the plain order)
  if constexpr (B0_EARLY) {
    if (nk > 0) {
      char* lb0 = smem + BM * 128 + wave * 1024;       // ring slot 0
      static_for<BJ>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if (j < BJ - 1 || lastb) {
          __builtin_amdgcn_global_load_lds((gptr_t)wptr[j], (lptr_t)(lb0 + j * (NW * 1024)), 16, 0, 0);
          wptr[j] += KT;
        }
      });
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int HWo = p.Hout * p.Wout;
  const int Hup = p.Hin << p.up, Wup = p.Win << p.up;
  // (prologue cost, tools/timeline_probe.py: the two integer divisions per tile row below took 1.5 - 2.7 k cycles of every launch.
  // Linear layers / 1x1 convs -- output row m IS source row m -- skip the pixel decomposition altogether; power-of-two image
  // sizes (every SDXL level) use shifts; anything else keeps the divisions.)
  const bool lin_rows = p.ksize == 1 && p.stride == 1 && p.up == 0 && p.pad == 0;
  const bool pow2 = (HWo & (HWo - 1)) == 0 && (p.Wout & (p.Wout - 1)) == 0;
  const int sh_hw = __builtin_ctz((unsigned)HWo | 0x40000000u), sh_w = __builtin_ctz((unsigned)p.Wout | 0x40000000u);
  int rb[AJ], ry[AJ], rx[AJ], rsw[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int row = (j * NW + wave) * 8 + lrow;
    const int m = m0 + row;
    rsw[j] = (slot ^ ((row >> 1) & 7)) * CE;
    rb[j] = m < p.M ? m : -1; ry[j] = 0; rx[j] = 0;          // lin_rows: rb carries the row itself
    if (!lin_rows) {
      if (m < p.M) {
        int b, rem, oy;
        const int ml = m - mph;      // (phase form: row inside the phase, entries of Hout x Wout = Hin x Win rows)
        if (pow2) { b = ml >> sh_hw; rem = ml & (HWo - 1); oy = rem >> sh_w; }
        else { b = ml / HWo; rem = ml - b * HWo; oy = rem / p.Wout; }
        rb[j] = b; ry[j] = oy * p.stride - pady; rx[j] = (rem - oy * p.Wout) * p.stride - padx;
      } else { rb[j] = -1; ry[j] = -(1 << 28); rx[j] = 0; }
    }
  }
  const T* Ag = reinterpret_cast<const T*>(p.A);
  const T* aptr[AJ];
  int aadv[AJ];
  int s_c0 = 0, s_dy = 0, s_dx = 0;
  if (kbeg > 0) {   // start the tap walk inside the contraction
    const int e0 = kbeg * KT, tap = e0 / p.Cin;
    s_c0 = e0 - tap * p.Cin; s_dy = tap / p.ksize; s_dx = tap - s_dy * p.ksize;
  }
  auto retap = [&]() {
    if (lin_rows) {       // one tap, rows are contiguous K-runs: no bounds / pixel arithmetic
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        const bool ok = rb[j] >= 0 && s_dy == 0;
        aptr[j] = ok ? Ag + (size_t)rb[j] * p.lda + rsw[j] + s_c0 : reinterpret_cast<const T*>(zeros);
        aadv[j] = ok ? KT : 0;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int iy = ry[j] + s_dy, ix = rx[j] + s_dx;
      const bool ok = (unsigned)iy < (unsigned)Hup && (unsigned)ix < (unsigned)Wup;
      const size_t off = (((size_t)(rb[j] < 0 ? 0 : rb[j]) * p.Hin + ((ok ? iy : 0) >> p.up)) * p.Win + ((ok ? ix : 0) >> p.up)) * p.lda + rsw[j] + s_c0;
      aptr[j] = ok ? Ag + off : reinterpret_cast<const T*>(zeros);
      aadv[j] = ok ? KT : 0;
    }
  };
  retap();
  // Linear layers (LIN; today = the fused cross-attention projections): scalar-base DMA addressing.  A row of the tile is a
  // contiguous K-run, so piece q reads {wave-uniform 64-bit base in SGPRs} + {loop-invariant 32-bit lane offset}: the k-loop
  // advances TWO scalar bases per k-tile (s_add_u32 / s_addc_u32) instead of PER 64-bit VGPR pointers (2 VALU each) and drops
  // the tap walk.  Rows past M read row M - 1 (never stored).
  unsigned long long abase = 0, wbase = 0;
  unsigned aoff[AJ], woff[BJ];
  if constexpr (LIN) {
    abase = (unsigned long long)(uintptr_t)(Ag + (size_t)m0 * p.lda + (size_t)kbeg * KT);
    wbase = (unsigned long long)(uintptr_t)(reinterpret_cast<const T*>(p.W) + (size_t)n0 * p.Kpad + (size_t)kbeg * KT);
    abase = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(abase >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)abase);
    wbase = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(wbase >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)wbase);
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      int row = (j * NW + wave) * 8 + lrow;
      const int sw = (slot ^ ((row >> 1) & 7)) * 16;
      if (m0 + row >= p.M) row = p.M - 1 - m0;
      aoff[j] = (unsigned)row * (unsigned)(p.lda * (int)sizeof(T)) + sw;
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int row = (j * NW + wave) * 8 + lrow;
      woff[j] = (unsigned)row * (unsigned)(p.Kpad * (int)sizeof(T)) + (slot ^ ((row >> 1) & 7)) * 16;
    }
  }
  // pieces q of one k-tile: q < AJ -> activation piece q, else weight piece q - AJ.  PH selects the pieces with q % 3 == PH
  // (PH < 0: all of them); the tap walk advances once per k-tile, after the last piece (tile_done).
  auto issue = [&](int buf, auto PH) {
    constexpr int ph = decltype(PH)::value;
    char* la = smem + buf * STAGE + wave * 1024;
    char* lb = la + BM * 128;
    static_for<PER>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      if constexpr (ph == -1 || (ph >= 0 && q % 3 == ph) || (ph == -3 && q < AJ)) {      // -1: all pieces; -3: the activation pieces only
        if constexpr (LIN) {
          // saddr form: global_load_lds_dwordx4 voffset, sbase -- M0 = LDS byte address of this wave's 1-KiB piece
          // (hand-written, so the hazards are ours to keep: an LDS-DMA instruction must not issue in the wait state right behind
          // the SALU write of M0 -- it would take the PREVIOUS piece's LDS address -- and a VMEM instruction needs 5 wait
          // states behind a VALU write (v_readlane / v_readfirstlane restore) of its scalar base; s_mov + s_nop 3 covers both.
          // The compiler's hazard recogniser does this for the builtin form and does not look inside inline asm.)
          if constexpr (q < AJ) {
            const unsigned m = lds0 + buf * STAGE + wave * 1024 + q * (NW * 1024), vo = aoff[q];
            const unsigned long long sb = abase;      // (asm operands do not capture into the generic lambda by themselves)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m), "v"(vo), "s"(sb) : "memory");
          } else if (q - AJ < BJ - 1 || lastb) {
            const unsigned m = lds0 + buf * STAGE + BM * 128 + wave * 1024 + (q - AJ) * (NW * 1024), vo = woff[q - AJ];
            const unsigned long long sb = wbase;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m), "v"(vo), "s"(sb) : "memory");
          }
        } else if constexpr (q < AJ) {
          __builtin_amdgcn_global_load_lds((gptr_t)aptr[q], (lptr_t)(la + q * (NW * 1024)), 16, 0, 0);
          aptr[q] += aadv[q];
        } else if (q - AJ < BJ - 1 || lastb) {     // ragged weight tile: wave-uniform predicate on the last piece
          __builtin_amdgcn_global_load_lds((gptr_t)wptr[q - AJ], (lptr_t)(lb + (q - AJ) * (NW * 1024)), 16, 0, 0);
          wptr[q - AJ] += KT;
        }
      }
    });
  };
  auto tile_done = [&]() {
    if constexpr (LIN) { abase += KT * sizeof(T); wbase += KT * sizeof(T); return; }
    s_c0 += KT;
    if (s_c0 == p.Cin) {
      s_c0 = 0;
      if (++s_dx == p.ksize) { s_dx = 0; ++s_dy; }
      retap();
    }
  };

  f32x16 acc[TM][TN];   // (zeroed behind the prologue's DMA issue: the writes ride under the ring fill)

  const int fr = lane & 31, fh = lane >> 5;
  // per-lane fragment address inside a stage: A rows wm*WM + i*32 + fr (i -> +4096 B immediate), B rows likewise behind
  // the A tile.  sw(row) = (row>>1)&7 is the same for rows 32 apart, so one base per operand; step kk flips chunk bits
  // 1..2:  chunk(kk) = (kk*2 + fh) ^ sw = (fh ^ sw) ^ (kk << 1)  ->  byte offset ^ (kk << 5)
  unsigned basea, baseb;
  {
    const int ra = wm * WM + fr, rbw = wn * WN + fr;
    basea = lds0 + ra * 128 + ((fh ^ ((ra >> 1) & 7)) << 4);
    baseb = lds0 + BM * 128 + rbw * 128 + ((fh ^ ((rbw >> 1) & 7)) << 4);
  }
  constexpr bool HL = is_hl<T>::value;        // split-operand element: four fragment sets (hi0, lo0, hi1, lo1), three MFMAs per pair
  frag_t fA[HL ? 4 : 2][TM], fB[HL ? 4 : 2][TN];
  auto ldfrag = [&](unsigned so, int kk, auto SET) {
    constexpr int set = decltype(SET)::value;
    const unsigned aa = (basea ^ (kk << 5)) + so, ab = (baseb ^ (kk << 5)) + so;
    static_for<TM>([&](auto I) { fA[set][decltype(I)::value] = lds_read128<decltype(I)::value * 4096, frag_t>(aa); });
    static_for<TN>([&](auto J) { fB[set][decltype(J)::value] = lds_read128<decltype(J)::value * 4096, frag_t>(ab); });
  };
  // MFMAs of one kk-step from fragment set SET; DMA pieces PH (or none, PH = 3) are issued between them
  auto mma = [&](auto SET, int buf, auto PH, bool more, auto SWT) {
    constexpr int set = decltype(SET)::value;
    constexpr int ph = decltype(PH)::value;
    constexpr bool sw = decltype(SWT)::value;      // operand roles swapped (TSW): D^T tiles
    if constexpr (!HL) {
    if constexpr (sw) acc[0][0] = PipeElem<T>::mma(fA[set][0], fB[set][0], acc[0][0]);
    else acc[0][0] = PipeElem<T>::mma(fB[set][0], fA[set][0], acc[0][0]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (ph < 3) {
      if (more) issue(buf, PH);            // wave-uniform branch around the DMA pieces only, never around MFMAs
      __builtin_amdgcn_sched_barrier(0);
    }
    static_for<TM * TN - 1>([&](auto X) {
      constexpr int x = decltype(X)::value + 1, i = x / TN, j = x % TN;
      if constexpr (sw) acc[i][j] = PipeElem<T>::mma(fA[set][i], fB[set][j], acc[i][j]);
      else acc[i][j] = PipeElem<T>::mma(fB[set][j], fA[set][i], acc[i][j]);
    });
    __builtin_amdgcn_sched_barrier(0);
    }
  };
  // split-operand MFMAs.  CROSS = false: hi x hi of fragment set SH (TM*TN MFMAs); CROSS = true: the two cross terms
  // w_hi x a_lo and w_lo x a_hi of the pair (SH, SL) (2*TM*TN MFMAs).  DMA pieces PH go behind the first MFMA, as above.
  // WX = every packed weight of this layer is ONE f16 (its lo half is zero: what a real SDXL record holds): the w_lo x a_hi
  // MFMAs would add exact zeros and are left out, as are the ds_reads of the weights' lo fragments -- bit-identical results.
  auto mma_hl = [&](auto SHI, auto SLO, auto CROSS, auto WXT, int buf, auto PH, bool more) {
    if constexpr (HL) {
      constexpr int sh = decltype(SHI)::value, sl = decltype(SLO)::value, ph = decltype(PH)::value;
      constexpr bool cross = decltype(CROSS)::value, wx = decltype(WXT)::value;
      auto one = [&](auto X) {
        constexpr int x = decltype(X)::value, i = x / TN, j = x % TN;
        if constexpr (!cross) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fB[sh][j], fA[sh][i], acc[i][j], 0, 0, 0);
        else {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fB[sh][j], fA[sl][i], acc[i][j], 0, 0, 0);
          if constexpr (!wx) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fB[sl][j], fA[sh][i], acc[i][j], 0, 0, 0);
        }
      };
      one(std::integral_constant<int, 0>{});
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (ph < 3) {
        if (more) issue(buf, PH);
        __builtin_amdgcn_sched_barrier(0);
      }
      static_for<TM * TN - 1>([&](auto X) { one(std::integral_constant<int, decltype(X)::value + 1>{}); });
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
  using IALL = std::integral_constant<int, -1>;
  using IAONLY = std::integral_constant<int, -3>;
  constexpr int LEAD = S2 ? NS - 2 : NS - 1;   // tile kt + LEAD is issued during tile kt
  constexpr int NPRO = LEAD;                   // tiles staged by the prologue
  static_assert(!S2 || (NS >= 4 && !HL), "two tiles per rendezvous: ring of >= 4 slots, f16 / f32 elements");

  // fused cross-attention, one-MFMA-row wave tiles: the 24 context fragments (96 VGPRs -- these kernels have the room) are
  // requested BEFORE the first DMA piece, so they are the oldest entries of the in-order vmcnt queue and ride under the
  // prologue's wait for tile 0 instead of adding a memory round trip to the epilogue
  constexpr bool XA_EARLY = XA && TM == 1 && !XH;      // (the split-precision form needs 48 fragments per head: loaded inside the epilogue)
  half8 xkf[XA ? 3 : 1][4], xvf[XA ? 2 : 1][6];
  if constexpr (XA_EARLY) xattn_load_frags(p, m0 + wm * WM, n0 + wn * WN, lane, xkf, xvf);
  // folded LayerNorm: the tile's row coefficients, evaluated once per workgroup (LnCoop) where 2 KiB of LDS are left behind the ring
  typedef LnCoop<BM, 64 * NW> LnC;
  constexpr bool LN_COOP = LnC::OK && pipe_lds_total(NS * STAGE, 0) > NS * STAGE;
  float* ln_coef = reinterpret_cast<float*>(smem + NS * STAGE);
  LnC lnc;
  if constexpr (LN_COOP) { lnc.load(p, m0, tid); __builtin_amdgcn_sched_barrier(0); }
  // ---- prologue: tiles 0 .. NPRO-1 in flight, wait for tile 0 only
#pragma unroll
  for (int s = 0; s < NPRO; ++s)
    if (s < nk) {
      if (B0_EARLY && s == 0) issue(0, IAONLY{}); else issue(s, IALL{});      // (tile 0's weight pieces are already on their way)
      tile_done();
    }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float lnA[TM], lnC[TM];
  bool hl_wexact = false;        // split-operand launches: every packed weight is one f16 (its lo half is zero)
  const bool ln_coop = LN_COOP && p.ln_slots <= 24;
  if constexpr (LN_COOP) lnc.finish(p, m0, ln_coef);
  if (!ln_coop) ln_prologue<TM>(p, m0 + wm * WM, fr, lnA, lnC);
  // (S2: the first rendezvous covers tiles 0 AND 1)
  if (NPRO <= nk) wait_tiles(std::integral_constant<int, NPRO - (S2 ? 2 : 1)>{}); else wait_vmcnt<0>();
  // finish()'s ds_write of the row coefficients must have LANDED before the barrier releases their readers: a raw s_barrier
  // carries no wait of its own, and a wave whose tile 0 is already there reaches it a few cycles behind the write
  if constexpr (LN_COOP) wait_lgkmcnt<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  if (ln_coop) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      lnA[i] = p.ln_stat ? ln_coef[(wm * WM + i * 32 + fr) * 2] : 1.f;
      lnC[i] = p.ln_stat ? ln_coef[(wm * WM + i * 32 + fr) * 2 + 1] : 0.f;
    }
  }
  if constexpr (HL) {   // split-operand weights are packed times a power of two (exact): the row coefficient of the epilogue undoes it
    // (the A operand's factor is per batch entry of the row: IgemmParams::a_scale_rpb)
    const float wsc = p.acc_scale ? *p.acc_scale : 1.f;                                           // powers of two: the products are exact
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * WM + i * 32 + fr;
      const int be = p.a_scale_rpb > 0 ? ((m < p.M ? m : p.M - 1) - mph) / p.a_scale_rpb : 0;      // (phase form: a_scale_rpb = source rows per entry)
      lnA[i] = wsc * (p.a_scale ? p.a_scale[be] : 1.f); lnC[i] = 0.f;
    }
    // (readfirstlane: the compiler must SEE that the choice is wave-uniform -- as a vector condition it runs both k-loops one after
    // the other under complementary EXEC masks, and MFMAs, barriers and the M0-addressed DMA do not honour EXEC)
    const int wx = (p.acc_scale && p.hl_wexact_ok && p.acc_scale[1] != 0.f) ? 1 : 0;
    hl_wexact = __builtin_amdgcn_readfirstlane(wx) != 0;
  }
  ldfrag(0, 0, I0{});
  // The k-loop is unrolled by the ring depth: ring slots become compile-time constants, so every
  // fragment read is {one of 16 loop-invariant lane addresses} + immediate and the DMA destinations fold into M0
  // constants -- the rolled loop re-derives them with ~25 VALU / SALU instructions per k-tile, and instruction issue (not
  // LDS or DMA bandwidth) is what fills this kernel's SIMDs.  ds_read immediates are 16 bit: slots
  // beyond 64 KiB go through a second address set (+ 65536).
  // wave tiles of up to 4 MFMA tiles per operand: two address sets (+0, +64 KiB); wider ones (256x160: 5): one set per slot
  constexpr bool PERSLOT = TM > 4 || TN > 4 || NS * STAGE > 131072;
  constexpr int NSET = PERSLOT ? NS : 2;
  unsigned fa[NSET][4], fb[NSET][4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int q = 0; q < NSET; ++q) {
      fa[q][kk] = (basea ^ (kk << 5)) + (PERSLOT ? q * STAGE : q * 65536u);
      fb[q][kk] = (baseb ^ (kk << 5)) + (PERSLOT ? q * STAGE : q * 65536u);
    }
  auto ldf = [&](auto SO, auto KK, auto SET, auto NOB) {          // NOB: leave out the weight fragments (split-operand lo sets of exact-f16 weights)
    constexpr unsigned so = decltype(SO)::value;
    constexpr int kk = decltype(KK)::value, set = decltype(SET)::value;
    constexpr bool nob = decltype(NOB)::value;
    constexpr int hi = PERSLOT ? (int)(so / STAGE) : (so >= 65536u ? 1 : 0);
    constexpr unsigned lo = PERSLOT ? 0u : so - hi * 65536u;
    static_assert(lo + (TM - 1) * 4096 < 65536u && lo + (TN - 1) * 4096 < 65536u, "fragment immediate out of range");
    static_for<TM>([&](auto I) { fA[set][decltype(I)::value] = lds_read128<lo + decltype(I)::value * 4096, frag_t>(fa[hi][kk]); });
    if constexpr (!nob) static_for<TN>([&](auto J) { fB[set][decltype(J)::value] = lds_read128<lo + decltype(J)::value * 4096, frag_t>(fb[hi][kk]); });
  };
  using NB0 = std::false_type;
  auto ktile = [&](int kt, auto CUR, auto WXT) {
    constexpr bool wx = decltype(WXT)::value;
    using WX = std::integral_constant<bool, wx>;
    constexpr int NFL = wx ? TM : NF;          // ds_reads of a lo fragment set
    constexpr int c = decltype(CUR)::value;
    constexpr int nslot = (c + 1) % NS, fl = (c + NS - (S2 ? 2 : 1)) % NS;      // fl: the slot tile kt + LEAD goes into
    using SO = std::integral_constant<unsigned, (unsigned)c * STAGE>;
    using SN = std::integral_constant<unsigned, (unsigned)nslot * STAGE>;
    const bool more = kt + LEAD < nk;
    if constexpr (HL) {
      // one 32-deep k-tile = the pairs (hi0, lo0) and (hi1, lo1) in sets 0..3; set 0 was requested behind the previous barrier
      using F = std::false_type; using Tt = std::true_type;
      ldf(SO{}, I1{}, I1{}, WX{});
      wait_lgkmcnt<NFL>();
      mma_hl(I0{}, I0{}, F{}, WX{}, fl, I0{}, more);      // w_hi0 x a_hi0
      ldf(SO{}, I2{}, I2{}, NB0{});
      wait_lgkmcnt<NF>();
      mma_hl(I0{}, I1{}, Tt{}, WX{}, fl, I1{}, more);     // w_hi0 x a_lo0 (+ w_lo0 x a_hi0)
      ldf(SO{}, I3{}, I3{}, WX{});
      wait_lgkmcnt<NFL>();
      mma_hl(I2{}, I2{}, F{}, WX{}, fl, I2{}, more);      // w_hi1 x a_hi1
      if (more) tile_done();
      if (kt + 1 < nk) {
        if (more) wait_tiles(std::integral_constant<int, NS - 2>{}); else wait_vmcnt<0>();
        wait_lgkmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        ldf(SN{}, I0{}, I0{}, NB0{});
      } else {
        wait_lgkmcnt<0>();
      }
      mma_hl(I2{}, I3{}, Tt{}, WX{}, fl, I3{}, false);    // w_hi1 x a_lo1 (+ w_lo1 x a_hi1)
      return;
    }
    using SWT = std::integral_constant<bool, !HL && wx>;     // (non-split kernels: the flag selects the operand-swapped copy, TSW)
    ldf(SO{}, I1{}, I1{}, NB0{});
    wait_lgkmcnt<NF>();
    mma(I0{}, fl, I0{}, more, SWT{});
    ldf(SO{}, I2{}, I0{}, NB0{});
    wait_lgkmcnt<NF>();
    mma(I1{}, fl, I1{}, more, SWT{});
    ldf(SO{}, I3{}, I1{}, NB0{});
    wait_lgkmcnt<NF>();
    mma(I0{}, fl, I2{}, more, SWT{});
    if (more) tile_done();
    if (kt + 1 < nk) {
      if (!S2 || (kt & 1)) {
        // own pieces of the next tile (S2: the next two) landed, then the rendezvous; tiles beyond may stay in flight
        if (more) wait_tiles(std::integral_constant<int, LEAD - (S2 ? 2 : 1)>{}); else wait_vmcnt<0>();
        wait_lgkmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        ldf(SN{}, I0{}, I0{}, NB0{});
      } else {
        // S2, even tile: tile kt + 1 was covered by the rendezvous of tile kt - 1 (or the prologue's) -- no wait, no barrier
        ldf(SN{}, I0{}, I0{}, NB0{});
        wait_lgkmcnt<NF>();
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      wait_lgkmcnt<0>();
    }
    mma(I1{}, fl, I3{}, false, SWT{});
  };
  int kt = 0;
  auto kloop = [&](auto WXT) {
    for (; kt + NS <= nk; kt += NS) static_for<NS>([&](auto S) { ktile(kt + decltype(S)::value, S, WXT); });
    static_for<NS - 1>([&](auto S) { if (kt + decltype(S)::value < nk) ktile(kt + decltype(S)::value, S, WXT); });
  };
  if constexpr (HL) {
    // two copies of the k-loop: the compiler moves the first fragments (asm ds_reads it believes complete) into each copy's
    // registers at the loop entry -- they must have LANDED before that (one LDS latency per launch)
    wait_lgkmcnt<0>();
    if (hl_wexact) kloop(std::true_type{}); else kloop(std::false_type{});       // wave-uniform: a device scalar next to the weight scale
  } else if constexpr (TSW) {
    // (two copies of the k-loop, as the split-operand kernel's: the choice is made wave-uniform for the compiler, and the first
    // fragments -- asm reads it believes complete -- must have landed before either copy takes them over)
    wait_lgkmcnt<0>();
    if (tsw_swapped) kloop(std::true_type{}); else kloop(std::false_type{});
  } else kloop(std::false_type{});
  __builtin_amdgcn_s_barrier();                    // every wave is done reading the ring: it becomes the staging area
  asm volatile("" ::: "memory");
  if constexpr (BN == 128) {
    if (SK > 1) {
      // ---- split-K combine inside the launch.  Every slice parks its fp32 accumulators in its slab (register order: 16-byte
      // stores, lane-contiguous), then ONE agent-scope release + ticket; the workgroup that draws the last ticket acquires
      // once and sums the SK slabs in slice order 0..SK-1 -- its own included, so the result does not depend on which slice
      // arrived last (bit-reproducible) -- and runs the normal epilogue.  Correct for any placement of the slices
      // (cdna_hip_programming.md section 6 guideline 16: plain stores -> vmcnt(0) -> barrier -> lane-0 release -> asm vmcnt(0)
      // -> relaxed agent ticket; consumer: acquire once -> barrier -> plain loads).  The last arriver re-arms the counter.
      constexpr int NV = TM * TN * 4;                                    // f32x4 vectors per lane
      f32x4* slab = reinterpret_cast<f32x4*>(p.splitk_ws) + ((size_t)tile_id * SK + slice) * (size_t)(NW * NV * 64);
      static_for<TM * TN>([&](auto X) {
        constexpr int x = decltype(X)::value, i = x / TN, j = x % TN;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // (round 4: write-through stores instead of plain stores + an agent-scope release -- the release writes the XCD's L2 back once per
          //  workgroup, 240 times per launch; the write-through pieces leave as they are issued and vmcnt(0) covers them: g_splitk_wt = 0 restores the fence)
          const f32x4 v = f32x4{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
          f32x4* dst = slab + (size_t)((wave * NV + x * 4 + q) * 64 + lane);
          if (p.splitk_wt) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
          else *dst = v;
        }
      });
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      volatile int* flag = reinterpret_cast<volatile int*>(smem + NS * STAGE - 16);   // inside the one LDS array, beyond the staging regions
      if (tid == 0) {
        if (!p.splitk_wt) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(p.splitk_cnt + tile_id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (unsigned)(SK - 1);
        if (last) {
          __hip_atomic_store(p.splitk_cnt + tile_id, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm for the next launch
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        *flag = last;
      }
      __syncthreads();
      if (!*flag) return;
      const f32x4* s0 = reinterpret_cast<const f32x4*>(p.splitk_ws) + (size_t)tile_id * SK * (size_t)(NW * NV * 64);
      static_for<TM * TN>([&](auto X) {
        constexpr int x = decltype(X)::value, i = x / TN, j = x % TN;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 sum = s0[(size_t)((wave * NV + x * 4 + q) * 64 + lane)];
          for (int sl = 1; sl < SK; ++sl) sum += s0[(size_t)sl * (NW * NV * 64) + (size_t)((wave * NV + x * 4 + q) * 64 + lane)];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][4 * q + r] = sum[r];
        }
      });
      __syncthreads();          // every wave has read the flag before the staging regions are written
    }
  }
  if constexpr (XA) {
    static_assert(TN == 2 && sizeof(T) == 2, "fused cross-attention: wave tile = one 64-wide head, f16");
    static_assert(NW * WM * WN * 4 <= NS * STAGE, "staging regions must fit the dead ring");
    if constexpr (XH) {
      static_assert(!XH || (XA && TM == 1), "split-precision fused cross-attention: XA kernels with one-MFMA-row wave tiles");
      xattn_inplace_hl<TM>(p, acc, m0 + wm * WM, n0 + wn * WN, lane, lnA, lnC, zeros);
    } else {
    if constexpr (!XA_EARLY) xattn_load_frags(p, m0 + wm * WM, n0 + wn * WN, lane, xkf, xvf);
    xattn_inplace<TM>(p, acc, m0 + wm * WM, n0 + wn * WN, lane, lnA, lnC, zeros, xkf, xvf);
    }
    IgemmParams pe = p;                       // bias and the LayerNorm affine went into q: the store adds nothing
    pe.bias = nullptr; pe.ln_stat = nullptr;
    if (!p.epi_staged && igemm_rows_ok<TM, TN, false>(pe, n0 + wn * WN))
      igemm_epilogue_rows<TM, TN, false>(pe, acc, m0 + wm * WM, n0 + wn * WN, lane, lnA, lnC, zeros);
    else
      igemm_epilogue_staged<TM, TN>(pe, acc, m0 + wm * WM, n0 + wn * WN, lane, smem + wave * (WM * WN * 4), lnA, lnC, zeros);
    return;
  }
  // whole wave tiles take the direct row-per-lane epilogue (registers -> permlane32 half swap -> 16-byte stores); tiles cut by N
  // or n_split, the transposed V^T part, GroupNorm-statistics producers and unaligned outputs keep the LDS-staged one.  The
  // choice depends on N / alignment only (never on the batch), and every wave makes it for itself (staging regions are private).
  // (GEGLU projections keep the staged epilogue in THIS kernel.  The general direct form, igemm_epilogue_rows<.., true>, was 23 - 50 us
  // slower on the 256x320 GEGLU kernel -- its residual / ebias / statistics arrays spilled next to 160 accumulator registers,
  // profiles/r03_epilogue_ab.txt; igemm_wide_kernel now has a GEGLU-only direct form of its own, igemm_epilogue_geglu_rows, one tile
  // at a time with the column vectors in LDS: 215 registers, no scratch, profiles/geglu_epilogue_ab.txt)
  if constexpr (TSW) {
    if (tsw_swapped) {
      igemm_epilogue_swapped<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, lane, ln_coop ? ln_coef + (wm * WM) * 2 : nullptr, zeros);
      return;
    }
  }
  if (!p.epi_staged && p.act != 1 && igemm_rows_ok<TM, TN, false>(p, n0 + wn * WN)) {
    igemm_epilogue_rows<TM, TN, false>(p, acc, m0 + wm * WM, n0 + wn * WN, lane, lnA, lnC, zeros);
    return;
  }
  constexpr bool FITS = NW * WM * WN * 4 <= NS * STAGE;        // full-width staging regions fit the dead ring
  if (FITS || p.act == 1) {
    const int region = p.act == 1 ? WM * (WN / 2) * 4 : WM * WN * 4;   // GEGLU halves the staged width
    if constexpr (BM == 256 && BN == 128 && NW == 8 && WGM == 4 && (sizeof(T) == 2 || HL)) {      // (f16, and -- round 6 -- the split-operand kernel: fp32 rows, same epilogue)
      static_assert(NW * WM * WN * 4 + 4096 <= NS * STAGE, "GroupNorm-statistics scratch must fit behind the staging regions");
      const GnCtx gc{smem + NW * WM * WN * 4, wave, wm, wn, m0, n0};
      igemm_epilogue_staged<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, lane, smem + wave * region, lnA, lnC, zeros, &gc);
    } else
    igemm_epilogue_staged<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, lane, smem + wave * region, lnA, lnC, zeros);
  } else {
    igemm_epilogue<TM, TN>(p, acc, m0 + wm * WM, n0 + wn * WN, fr, fh, lnA, lnC);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Wide-tile variant for the GEGLU projections: block tile 256 x 320, k-tile 32.
//
// The global->LDS path sustains ~22 B/clk/CU whatever issues it, so the reachable MFMA rate of a tile is
// BM*BN/(BM+BN) flop per DMA byte: 85 for 256x128, 98 for 256x160, 142 for 256x320.  A 64-deep k-tile of that tile
// would not fit a 3-slot ring (72 KiB per slot); with KT = 32 a slot is 36 KiB and FOUR slots fit (144 KiB).  N = 10240 at
// M = 2048 is then 8 x 32 = 256 tiles: one workgroup per CU, ONE round (256x160 needs two, 256x128 three), so the per-tile
// fixed cost is paid once.  8 waves as 4 (M) x 2 (N), wave tile 64 x 160 = 2 x 5 MFMA tiles: 7 ds_read_b128 per 10 MFMA.
// LDS rows are 64 bytes (32 halfs): a 1-KiB DMA piece covers 16 rows, source chunk = slot ^ ((row>>2)&3), which makes the
// 16-lane ds_read_b128 service groups hit 16 distinct 16-byte slots of the 256-byte bank row.
// Per k-tile: {frags kk=0 -> 10 MFMA} {frags kk=1 -> wait own pieces of tile kt+1 -> barrier -> 10 MFMA with the pieces of
// tile kt+NS (slot just freed) issued between them}.  GEGLU epilogue only, in two 32-row passes: DIRECT = from the registers to 16-byte f16
// stores with the tile's column vectors in 2.5 KiB of static LDS (launch_wide: aligned f16 output, nothing but bias and the folded LayerNorm --
// every GEGLU projection of the UNet; tail 12.1 k cycles against 17.2 k, profiles/geglu_epilogue_timeline.txt), else staged through LDS.
#ifdef SDXL_MEASURE
// coarse s_memtime stamps of the wide kernel (tools/wide_timeline.py): [workgroup][wave][16], words 0..7 = entry, ring fill issued, tile 0 landed
// (first barrier passed), k-loop done, ring dead (barrier), first / second epilogue pass issued, stores drained
__device__ unsigned* g_wide_tl = nullptr;
void igemm_set_wide_timeline(void* buf) {
  unsigned* b = reinterpret_cast<unsigned*>(buf);
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_wide_tl), &b, sizeof(b)) != hipSuccess) throw std::runtime_error("igemm: cannot set the wide-kernel timeline buffer");
}
#define WIDE_STAMP(i) do { wtl[i] = (unsigned)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define WIDE_STAMP(i) do { } while (0)
#endif
// DB (round 5): fragments of the NEXT kk-step are requested before the MFMAs of the current one (two register sets, counted lgkmcnt, the pipe
// kernels' scheme): the rolled form above waits for its seven ds_read_b128 in front of every 10-MFMA burst with nothing of its own to issue
// meanwhile -- 1.85 - 1.97 k cycles per 32-deep k-tile for 1.28 k cycles of matrix-pipe work (profiles/r04_wide_geglu_timeline.txt).
template <int NS, bool DB = false, bool DIRECT = false>
__global__ __launch_bounds__(512) void igemm_wide_kernel(const IgemmParams p, const void* zeros) {
#ifdef SDXL_MEASURE
  unsigned wtl[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  wtl[8] = (unsigned)__builtin_amdgcn_s_memrealtime();     // 100 MHz constant clock: shader clock of this launch = d(memtime) / d(realtime)
#endif
  WIDE_STAMP(0);
  kernarg_prefetch<(int)sizeof(IgemmParams) + 8>();   // every argument line in flight at once (one wait instead of five)
  constexpr int BM = 256, BN = 320, KT = 32;
  constexpr int WM = 64, WN = 160, TM = 2, TN = 5, NF = TM + TN;
  constexpr int ROWB = KT * 2;                 // 64 bytes per tile row
  constexpr int STAGE = (BM + BN) * ROWB;      // 36864
  constexpr int AJ = BM / 16 / 8;              // 2 pieces of 16 rows per wave
  constexpr int BPC = BN / 16, BJ = (BPC + 7) / 8, REM = BPC % 8;   // 20 pieces: waves 0..3 carry 3, waves 4..7 carry 2
  constexpr int PER = AJ + BJ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const bool lastb = wave < REM;

  const int tilesN = (p.N + BN - 1) / BN;
  const int tilesM = (p.M + BM - 1) / BM;
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  int tm, tn;
  if ((size_t)p.N * p.K > (size_t)p.M * p.Cin) { tn = bid / tilesM; tm = bid - tn * tilesM; }
  else { tm = bid / tilesN; tn = bid - tm * tilesN; }
  const int m0 = tm * BM, n0 = tn * BN;
  auto wait_tiles = [&](auto KK) {
    constexpr int k = decltype(KK)::value;
    if (lastb) wait_vmcnt<PER * k>(); else wait_vmcnt<(PER - 1) * k>();
  };

  // ---- DMA geometry (linear layers only: ksize 1, stride 1): piece j of this wave = tile rows (j*8 + wave)*16 .. +15
  const int lrow = lane >> 2, slot = lane & 3;
  const half_t* aptr[AJ];
  int aadv[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int row = (j * 8 + wave) * 16 + lrow;
    const int m = m0 + row;
    const bool ok = m < p.M;
    aptr[j] = ok ? reinterpret_cast<const half_t*>(p.A) + (size_t)m * p.lda + (slot ^ ((row >> 2) & 3)) * 8
                 : reinterpret_cast<const half_t*>(zeros);
    aadv[j] = ok ? KT : 0;
  }
  const half_t* wptr[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int row = (j * 8 + wave) * 16 + lrow;
    wptr[j] = reinterpret_cast<const half_t*>(p.W) + (size_t)(n0 + row) * p.Kpad + (slot ^ ((row >> 2) & 3)) * 8;
  }
  auto issue = [&](int buf, auto Q) {            // piece Q of the next tile into ring slot buf
    constexpr int q = decltype(Q)::value;
    char* la = smem + buf * STAGE + wave * 1024;
    char* lb = la + BM * ROWB;
    if constexpr (q < AJ) {
      __builtin_amdgcn_global_load_lds((gptr_t)aptr[q], (lptr_t)(la + q * 8192), 16, 0, 0);
      aptr[q] += aadv[q];
    } else if (q - AJ < BJ - 1 || lastb) {
      __builtin_amdgcn_global_load_lds((gptr_t)wptr[q - AJ], (lptr_t)(lb + (q - AJ) * 8192), 16, 0, 0);
      wptr[q - AJ] += KT;
    }
  };

  // the two 32-row halves of the wave tile live in SEPARATE accumulator arrays: the epilogue runs once per half, and handing
  // it `&acc[i]` of one [2][5] array made hipcc address the accumulators through scratch (the round-1 build of this kernel
  // lost 35 us in its epilogue to exactly that)
  f32x16 acc0[1][TN], acc1[1][TN];
  const int nk = p.Kpad / KT;
  const int fr = lane & 31, fh = lane >> 5;
  unsigned basea, baseb;
  {
    const int ra = wm * WM + fr, rbw = wn * WN + fr;
    basea = lds0 + ra * ROWB + ((fh ^ ((ra >> 2) & 3)) << 4);
    baseb = lds0 + BM * ROWB + rbw * ROWB + ((fh ^ ((rbw >> 2) & 3)) << 4);
  }
  constexpr int NSET = DB ? 2 : 1;
  half8 fA[NSET][TM], fB[NSET][TN];
  auto ldfrag = [&](auto SET, unsigned so, int kk) {       // chunk(kk) = (kk*2 + fh) ^ sw = (fh ^ sw) ^ (kk << 1) -> byte offset ^ (kk << 5)
    constexpr int set = decltype(SET)::value;
    const unsigned aa = (basea ^ (kk << 5)) + so, ab = (baseb ^ (kk << 5)) + so;
    static_for<TM>([&](auto I) { fA[set][decltype(I)::value] = lds_read128<decltype(I)::value * 32 * ROWB>(aa); });
    static_for<TN>([&](auto J) { fB[set][decltype(J)::value] = lds_read128<decltype(J)::value * 32 * ROWB>(ab); });
  };
  using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, NSET - 1>;
  // ten MFMAs of one kk-step; with DMA: the PER pieces of the next tile go behind MFMAs 0, 2, 4, 6, 8
  auto mma = [&](auto SET, int buf, bool dma) {
    constexpr int set = decltype(SET)::value;
    __builtin_amdgcn_s_setprio(1);
    static_for<TM * TN>([&](auto X) {
      constexpr int x = decltype(X)::value, i = x / TN, j = x % TN;
      if constexpr (i == 0) acc0[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fB[set][j], fA[set][0], acc0[0][j], 0, 0, 0);
      else acc1[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fB[set][j], fA[set][1], acc1[0][j], 0, 0, 0);
      if constexpr ((x & 1) == 0 && x / 2 < PER) {
        __builtin_amdgcn_sched_barrier(0);
        if (dma) issue(buf, std::integral_constant<int, x / 2>{});
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };

  // folded LayerNorm: the tile's 256 row coefficients once per workgroup (LnCoop, 2 KiB of LDS behind the ring)
  typedef LnCoop<BM, 512> LnC;
  float* ln_coef = reinterpret_cast<float*>(smem + NS * STAGE);
  LnC lnc;
  lnc.load(p, m0, tid);
  // the tile's 320 columns of bias and ln_cs (value and gate halves interleaved by 16, as packed), once per workgroup: threads 0..79 /
  // 80..159 request 16 bytes each -- an absent vector reads the zero page -- BEFORE the first DMA piece like the statistics above (oldest
  // entries of the vmcnt queue: the ring's counted waits cover them), and park them in LDS behind the prologue's barrier.  The direct
  // epilogue reads them there in the accumulator layout instead of five dependent global round trips per pass.  (DIRECT only: the staged
  // instantiation has no such corner and loads nothing.)
  __shared__ __attribute__((aligned(16))) float cvec[2][DIRECT ? BN : 4];
  f32x4 cvv = {0.f, 0.f, 0.f, 0.f};
  if constexpr (DIRECT) {
    const bool cv_ln = tid >= BN / 4;
    const float* cv_src = cv_ln ? (p.ln_stat ? p.ln_cs : nullptr) : p.bias;
    cvv = *((cv_src && tid < BN / 2) ? reinterpret_cast<const f32x4*>(cv_src + n0 + 4 * (cv_ln ? tid - BN / 4 : tid))
                                      : reinterpret_cast<const f32x4*>(zeros));
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- prologue: NS - 1 tiles in flight, wait for tile 0 only.  The last ring slot is filled from inside k-tile 0 (its first kk-step
  // carries the pieces of tile NS - 1): the first MFMA does not wait behind the issue of a whole ring (every wave's VMEM issue queues
  // behind the CU's fetch rate: entry -> "ring fill issued" was 7.5 - 9 k cycles with three tiles, profiles/r04_wide_geglu_timeline.txt)
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) static_for<PER>([&](auto Q) { issue(s, Q); });
  WIDE_STAMP(1);
  float lnA[TM], lnC[TM];
  const bool ln_coop = p.ln_slots <= 24;
  lnc.finish(p, m0, ln_coef);
  if constexpr (DIRECT) {
    if (tid < BN / 2) *reinterpret_cast<f32x4*>(&cvec[0][0] + 4 * tid) = cvv;
  }
  if (!ln_coop) ln_prologue<TM>(p, m0 + wm * WM, fr, lnA, lnC);
  if (NS - 1 <= nk) wait_tiles(std::integral_constant<int, NS - 2>{}); else wait_vmcnt<0>();
  wait_lgkmcnt<0>();                             // the coefficients' ds_write has landed (raw s_barrier waits for nothing)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  WIDE_STAMP(2);
  if (ln_coop) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      lnA[i] = p.ln_stat ? ln_coef[(wm * WM + i * 32 + fr) * 2] : 1.f;
      lnC[i] = p.ln_stat ? ln_coef[(wm * WM + i * 32 + fr) * 2 + 1] : 0.f;
    }
  }
  // (zeroed only now: keeping 160 accumulator registers live across the statistics loads of ln_prologue spills)
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[0][j][r] = 0.f; acc1[0][j][r] = 0.f; }
  int cur = 0;
  if constexpr (DB) {
    // set 0 = kk-step 0, set 1 = kk-step 1 of the current tile.  Per tile: {request set 1 | wait set 0 | 10 MFMAs} {own pieces of tile kt + 1,
    // lgkmcnt(0) = every read of tile kt complete, barrier | request set 0 of tile kt + 1 | 10 MFMAs + the pieces of tile kt + NS}
    ldfrag(S0{}, 0, 0);
    wait_lgkmcnt<0>();       // (the compiler believes an asm read complete when the statement ends: nothing in flight across the loop entry)
    for (int kt = 0; kt < nk; ++kt) {
      const unsigned so = cur * STAGE;
      const int nxt = cur + 1 == NS ? 0 : cur + 1;
      ldfrag(S1{}, so, 1);
      wait_lgkmcnt<NF>();                         // set 0 has landed (the seven reads just issued may still be in flight)
      if (kt == 0) mma(S0{}, NS - 1, NS - 1 < nk); else mma(S0{}, cur, false);
      const bool more = kt + NS < nk;
      if (kt + 1 < nk) {
        if (kt + NS - 1 < nk) wait_tiles(std::integral_constant<int, NS - 2>{}); else wait_vmcnt<0>();
        wait_lgkmcnt<0>();                        // set 1 has landed: all of this wave's reads of tile kt are complete
        __builtin_amdgcn_s_barrier();             // tile kt+1 visible; slot of tile kt free for tile kt+NS
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(S0{}, nxt * STAGE, 0);             // in flight under the MFMAs of kk-step 1
      } else {
        wait_lgkmcnt<0>();
      }
      mma(S1{}, cur, more);
      cur = nxt;
    }
    wait_lgkmcnt<0>();
  } else
  for (int kt = 0; kt < nk; ++kt) {
    const unsigned so = cur * STAGE;
    ldfrag(S0{}, so, 0);
    wait_lgkmcnt<0>();
    if (kt == 0) mma(S0{}, NS - 1, NS - 1 < nk); else mma(S0{}, cur, false);      // (k-tile 0 completes the ring: slot NS - 1 has never been read)
    ldfrag(S0{}, so, 1);
    wait_lgkmcnt<0>();                          // own reads of tile kt complete
    const bool more = kt + NS < nk;
    if (kt + 1 < nk) {
      if (kt + NS - 1 < nk) wait_tiles(std::integral_constant<int, NS - 2>{}); else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();             // tile kt+1 visible; slot of tile kt free for tile kt+NS
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
    mma(S0{}, cur, more);
    cur = cur + 1 == NS ? 0 : cur + 1;
  }
  WIDE_STAMP(3);
  __builtin_amdgcn_s_barrier();                  // ring dead -> staging area
  asm volatile("" ::: "memory");
  WIDE_STAMP(4);
  if constexpr (DIRECT) {
    // aligned f16 output without residual, ebias or statistics (launch_wide checks: every GEGLU projection of the UNet): registers ->
    // 16-byte stores, one 32-row half at a time like the staged passes; rows past M are computed on zero-page operands and not stored
    const int mw = m0 + wm * WM, nwo = (n0 + wn * WN) >> 1;
    igemm_epilogue_geglu_rows<TN>(p, acc0, mw, nwo, lane, lnA[0], lnC[0], &cvec[0][wn * WN], &cvec[1][wn * WN]);
    WIDE_STAMP(5);
    igemm_epilogue_geglu_rows<TN>(p, acc1, mw + 32, nwo, lane, lnA[1], lnC[1], &cvec[0][wn * WN], &cvec[1][wn * WN]);
  } else if (p.act == 1) {
    // two passes of 32 rows: a full 64 x 80 fp32 staging region per wave would not fit next to seven others
    char* region = smem + wave * (32 * (WN / 2) * 4);
    {
      const float la1[1] = {lnA[0]}, lc1[1] = {lnC[0]};
      igemm_epilogue_staged_impl<1, TN, true>(p, acc0, m0 + wm * WM, n0 + wn * WN, lane, region, false, la1, lc1, zeros);
    }
    WIDE_STAMP(5);
    {
      const float la1[1] = {lnA[1]}, lc1[1] = {lnC[1]};
      igemm_epilogue_staged_impl<1, TN, true>(p, acc1, m0 + wm * WM + 32, n0 + wn * WN, lane, region, false, la1, lc1, zeros);
    }
  }   // (the launcher only admits GEGLU projections)
#ifdef SDXL_MEASURE
  WIDE_STAMP(6);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  WIDE_STAMP(7);
  wtl[9] = (unsigned)__builtin_amdgcn_s_memrealtime();
  if (g_wide_tl && lane == 0) {
#pragma unroll
    for (int i = 0; i < 10; ++i) g_wide_tl[((size_t)blockIdx.x * 8 + wave) * 16 + i] = wtl[i];
  }
#endif
}

// Per-DEVICE state: the zero page the DMA reads halo / tail rows from (GEMM and attention kernels alike) lives on the device that launches (the dynamic-LDS
// attribute, up to 147 KiB, is per (kernel, device) too: set_max_dynamic_lds).  A second sdxl_ctx on another GPU of the same
// process gets its own.
static const void* g_zero_pages[kMaxDevices] = {};
static int current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) throw std::runtime_error("igemm: no current HIP device");
  return d;
}
const void* igemm_zero_page() { return g_zero_pages[current_device()]; }
int igemm_current_device() { return current_device(); }
void igemm_glds_init() {
  const int d = current_device();
  if (g_zero_pages[d]) return;
  void* z = nullptr;
  if (hipMalloc(&z, 4096) != hipSuccess || hipMemset(z, 0, 4096) != hipSuccess)
    throw std::runtime_error("igemm: cannot allocate the zero page");
  g_zero_pages[d] = z;
}

// ---- launchers: a choice of igemm_select (select.cpp) -> its template instantiation.  Nothing here looks at the shape.
template <int BM, int BN, int NS, int MINB = 2>
static void launch_glds(const IgemmParams& p, const IgemmChoice& c, hipStream_t s) {
  const int dev = current_device();
  set_max_dynamic_lds<&igemm_glds_kernel<BM, BN, NS, MINB>>(c.lds, dev);
  hipLaunchKernelGGL((igemm_glds_kernel<BM, BN, NS, MINB>), dim3(c.grid), dim3(c.block), c.lds, s, p, g_zero_pages[dev]);
}

template <int BM, int BN, int NS, int WGM = 4, int NW = 8, typename T = half_t, bool XA = false, bool S2 = false, bool TSW = false, bool XH = false>
static void launch_pipe(const IgemmParams& p, const IgemmChoice& c, hipStream_t s) {
  // (the kernel carves the ring + LayerNorm coefficients out of its template arguments)
  if (c.lds != pipe_lds_total(NS * (BM + BN) * 128, 0) || c.block != 64 * NW) throw std::logic_error("igemm: choice and kernel disagree on the LDS layout");
  const int dev = current_device();
  set_max_dynamic_lds<&igemm_pipe_kernel<BM, BN, NS, WGM, NW, T, XA, S2, TSW, XH>>(c.lds, dev);
  if (c.splitk > 1 && (size_t)c.grid * BM * BN * 4 > p.splitk_ws_bytes) throw std::runtime_error("igemm: split-K workspace too small");
  hipLaunchKernelGGL((igemm_pipe_kernel<BM, BN, NS, WGM, NW, T, XA, S2, TSW, XH>), dim3(c.grid), dim3(c.block), c.lds, s, p, g_zero_pages[dev]);
}

static void launch_wide(const IgemmParams& p, const IgemmChoice& c, hipStream_t s) {
  const int dev = current_device();
#ifdef SDXL_MEASURE
  // register-double-buffered fragment reads (DB): measured on the bench line A/B/A/B, 21.213 / 21.179 (DB) vs 21.209 / 21.190 ms per step -- no
  // difference (profiles/r05_wide_double_buffer_ab.txt): the k-tile is LDS-bandwidth + matrix-pipe co-bound (112 KiB of fragment reads + 36 KiB of
  // DMA writes = 1156 LDS cycles against 1280 MFMA cycles), not latency-bound.  Measure builds only.
  if (c.db) {
    set_max_dynamic_lds<&igemm_wide_kernel<3, true>>(c.lds, dev);
    hipLaunchKernelGGL((igemm_wide_kernel<3, true>), dim3(c.grid), dim3(c.block), c.lds, s, p, g_zero_pages[dev]);
    return;
  }
#endif
  // the direct epilogue's case -- an aligned f16 output of whole column tiles that takes nothing but bias and the folded LayerNorm: every GEGLU
  // projection of the UNet -- has an instantiation of its own (both forms in one kernel spill next to the 160 accumulator registers).  Everything
  // else (the fp32 / HL16 outputs of the op entries and the mixed modes, an unaligned C) and igemm_epilogue_staged = 1, the A/B and identity
  // partner, run the staged instantiation.  Properties of the launch alone: never of M or the batch.
  const bool direct = !p.epi_staged && p.act == 1 && !p.R && !p.stat_out && !p.gn_part && !p.ebias && p.c_dt == DT_F16 && p.N % 320 == 0 &&
                      (p.ldc & 7) == 0 && (reinterpret_cast<uintptr_t>(p.C) & 15) == 0;
  if (direct) {
    set_max_dynamic_lds<&igemm_wide_kernel<3, false, true>>(c.lds, dev);
    hipLaunchKernelGGL((igemm_wide_kernel<3, false, true>), dim3(c.grid), dim3(c.block), c.lds, s, p, g_zero_pages[dev]);
    return;
  }
  set_max_dynamic_lds<&igemm_wide_kernel<3, false>>(c.lds, dev);
  hipLaunchKernelGGL((igemm_wide_kernel<3, false>), dim3(c.grid), dim3(c.block), c.lds, s, p, g_zero_pages[dev]);
}

// Context K [B][n_ctx][C] / V^T [B][C][vt_ld] (f16) -> the operand-order image the fused cross-attention reads: per (batch entry, head)
// NB = ceil(n_ctx / 96) blocks of 24 fragments of 64 lanes x 8 halfs; block blk holds keys 96 blk .. + 95 -- 12 fragments of K (key tile t,
// k-step s4: key = 96 blk + 32t + lane&31, d = 16 s4 + 8(e>>2) + 4(lane>>5) + (e&3)) then 12 of V^T (d tile dt, k-step s6: d = 32dt + lane&31,
// key = 96 blk + 16 s6 + 8(e>>2) + 4(lane>>5) + (e&3)); keys >= n_ctx are zero.  n_ctx <= 96: one block, the image xattn_inplace and xattn_unit
// read; more blocks are read by xattn_unit_long (igemm_wreg.hip) alone.
__global__ void xattn_pack_kernel(const half_t* K, const half_t* Vt, half8* out, int B, int C, int nctx, int vt_ld) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int H = C >> 6, NB = (nctx + 95) / 96;
  if (i >= (size_t)B * H * NB * 24 * 64) return;
  const int lane = (int)(i & 63), f = (int)((i >> 6) % 24);
  const int bhb = (int)(i / (24 * 64)), bh = bhb / NB, k0 = 96 * (bhb - bh * NB), b = bh / H, h = bh - b * H;
  const int fr = lane & 31, fh = lane >> 5;
  half8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int sub = 8 * (e >> 2) + 4 * fh + (e & 3);
    half_t x = (half_t)0.f;
    if (f < 12) {
      const int key = k0 + 32 * (f >> 2) + fr, d = 16 * (f & 3) + sub;
      if (key < nctx) x = K[((size_t)b * nctx + key) * C + h * 64 + d];
    } else {
      const int g = f - 12, d = 32 * (g / 6) + fr, key = k0 + 16 * (g % 6) + sub;
      if (key < nctx) x = Vt[((size_t)b * C + h * 64 + d) * vt_ld + key];
    }
    v[e] = x;
  }
  out[i] = v;
}
size_t xattn_pack_bytes(int B, int C, int n_ctx) { return (size_t)B * (C / 64) * ((n_ctx + 95) / 96) * 24 * 64 * 16; }
void launch_xattn_pack(const void* K, const void* Vt, void* out, int B, int C, int nctx, int vt_ld, hipStream_t s) {
  const size_t n = xattn_pack_bytes(B, C, nctx) / 16;
  if (n == 0) return;
  hipLaunchKernelGGL(xattn_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const half_t*>(K),
                     reinterpret_cast<const half_t*>(Vt), reinterpret_cast<half8*>(out), B, C, nctx, vt_ld);
}

void launch_igemm_dma(const IgemmParams& p, const IgemmChoice& c, hipStream_t s) {
#define PIPE(BM, BN, NS, WGM, NW, T, DT, XA, S2, TSW, XH)                                                                                 \
  if (c.family == IG_PIPE && c.bm == BM && c.bn == BN && c.ns == NS && c.wgm == WGM && c.nw == NW && c.elem == DT && c.xa == XA && c.s2 == S2 && c.tsw == TSW && c.xh == XH) \
    return launch_pipe<BM, BN, NS, WGM, NW, T, XA, S2, TSW, XH>(p, c, s)
  PIPE(96, 128, 3, 3, 6, half_t, DT_F16, true, false, false, true);      // fused cross-attention: split-precision form, f16 form
  PIPE(128, 128, 4, 4, 8, half_t, DT_F16, true, false, false, true);
  PIPE(256, 128, 3, 4, 8, half_t, DT_F16, true, false, false, false);
  PIPE(128, 128, 4, 4, 8, half_t, DT_F16, true, false, false, false);
  PIPE(128, 128, 5, 4, 8, half_t, DT_F16, true, false, false, false);
  PIPE(96, 128, 3, 3, 6, half_t, DT_F16, true, false, false, false);
  PIPE(256, 128, 3, 4, 8, half_t, DT_F16, false, false, false, false);
  if (c.family == IG_GLDS && c.bm == 128 && c.bn == 128 && c.ns == 2) return launch_glds<128, 128, 2>(p, c, s);
  if (c.family == IG_GLDS && c.bm == 64 && c.bn == 128 && c.ns == 2) return launch_glds<64, 128, 2>(p, c, s);
  PIPE(256, 128, 3, 4, 8, half_t, DT_F16, false, false, true, false);
  PIPE(128, 128, 4, 4, 8, half_t, DT_F16, false, false, false, false);
  PIPE(256, 160, 3, 8, 8, half_t, DT_F16, false, false, false, false);
  PIPE(128, 128, 5, 4, 8, half_t, DT_F16, false, false, false, false);
  PIPE(96, 128, 5, 3, 6, half_t, DT_F16, false, false, false, false);
  PIPE(96, 128, 4, 3, 6, half_t, DT_F16, false, false, false, false);
  PIPE(96, 128, 5, 3, 6, half_t, DT_F16, false, true, false, false);
  PIPE(128, 160, 3, 4, 4, half_t, DT_F16, false, false, false, false);
  if (c.family == IG_WIDE && c.bm == 256 && c.bn == 320 && c.ns == 3) return launch_wide(p, c, s);
  PIPE(256, 128, 3, 4, 8, float, DT_F32, false, false, false, false);
  PIPE(128, 128, 4, 4, 8, float, DT_F32, false, false, false, false);
  PIPE(96, 128, 5, 3, 6, hl16_t, DT_HL, false, false, false, false);
  PIPE(256, 128, 3, 4, 8, hl16_t, DT_HL, false, false, false, false);
  PIPE(128, 160, 3, 4, 4, hl16_t, DT_HL, false, false, false, false);
  PIPE(128, 128, 4, 4, 8, hl16_t, DT_HL, false, false, false, false);
#undef PIPE
  throw std::logic_error("igemm: the selection chose a direct-to-LDS kernel that is not instantiated");
}

}  // namespace sdxl
