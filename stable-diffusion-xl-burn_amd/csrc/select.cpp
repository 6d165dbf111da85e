// Which kernel a GEMM or attention call runs on -- decided here, once, and nowhere else.  Plain host C++: integer arithmetic on the
// fields of IgemmParams / AttnParams (pointers are read for null-ness and alignment only) and on a SelectKnobs value; no HIP call, no
// global.  The launchers (igemm.hip, igemm_glds.hip, igemm_wreg.hip, attention.hip) map the returned choice to a template
// instantiation and launch it; run_conv's predicates (igemm_gn_part_ok, igemm_wreg_selected, igemm_wreg_xattn_selected) read the
// same rules.  The choice decides speed AND output bits (the weights-in-registers kernel, the in-launch split-K and the epilogue
// GroupNorm statistics each sum or round in their own order), so every rule that can change bits is a function of ONE batch
// entry's shape (rows per entry, N, K) -- never of the batch size: an entry comes out bit-identical whether it runs alone, in the
// CFG pair or in a larger batch (tests/test_cpu_select.py on the CPU, tests/test_gpu_fullsize.py end to end).  DESIGN.md 3.3.
#include "kernels.h"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <stdexcept>

namespace sdxl {

// ---------------------------------------------------------------------------------------------------------
// knobs: one table (key of sdxl_debug_set, field, default = the field's initialiser in kernels.h)
namespace {
struct KnobSlot { const char* key; int SelectKnobs::*field; };
constexpr KnobSlot kKnobSlots[] = {
    {"igemm_variant", &SelectKnobs::igemm_variant}, {"igemm_wreg", &SelectKnobs::igemm_wreg}, {"wreg_xattn", &SelectKnobs::wreg_xattn},
    {"hl_tile96", &SelectKnobs::hl_tile96},         {"igemm_tsw", &SelectKnobs::igemm_tsw},   {"wide_db", &SelectKnobs::wide_db},
    {"attn_variant", &SelectKnobs::attn_variant},   {"attn_xsplit", &SelectKnobs::attn_xsplit},
#ifdef SDXL_MEASURE
    {"igemm_unrolled", &SelectKnobs::igemm_unrolled},
#endif
};
constexpr int kNumKnobs = sizeof(kKnobSlots) / sizeof(kKnobSlots[0]);
struct KnobStore {
  std::atomic<int> v[kNumKnobs];
  KnobStore() { const SelectKnobs d; for (int i = 0; i < kNumKnobs; ++i) v[i] = d.*kKnobSlots[i].field; }
};
KnobStore g_knobs;
}  // namespace
bool select_knob_set(const char* key, int value) {
  for (int i = 0; i < kNumKnobs; ++i)
    if (std::strcmp(key, kKnobSlots[i].key) == 0) { g_knobs.v[i] = value; return true; }
  return false;
}
SelectKnobs select_knobs_snapshot() {
  SelectKnobs k;
  for (int i = 0; i < kNumKnobs; ++i) k.*kKnobSlots[i].field = g_knobs.v[i].load();
  return k;
}

// ---------------------------------------------------------------------------------------------------------
// GEMM
namespace {
bool xattn_forced_pipe(int v) { return v == 35 || v == 36 || v == 44 || v == 45; }      // forced numbers that keep a fused cross-attention on a pipe tile
bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
bool is_linear(const IgemmParams& p) { return p.ksize == 1 && p.stride == 1 && p.up == 0; }

// The tiles of the release library by their variant number (sdxl_debug_set "igemm_variant"; tools, profiles and DESIGN.md cite the
// numbers).  wgm: waves along M; w: the cost model's weight of the tile (0 = never a candidate of the automatic choice).
struct Tile { int number, family, bm, bn, ns, wgm, nw, s2; double w; };
constexpr Tile kTiles[] = {
    {4, IG_GLDS, 128, 128, 2, 2, 4, 0, 0.0},     // 4 waves, 2-3 co-resident blocks: ragged multi-round grids
    {6, IG_GLDS, 64, 128, 2, 2, 4, 0, 0.0},
    {35, IG_PIPE, 256, 128, 3, 4, 8, 0, 1.0},    // 8 waves, hand-ordered k-loop unrolled by the ring depth; outputs with a transposed part (fused QKV: V^T) take the operand-swap twin
    {36, IG_PIPE, 128, 128, 4, 4, 8, 0, 1.0},
    {38, IG_PIPE, 256, 160, 3, 8, 8, 0, 1.2},    // 256x160 GEGLU tile (8x1 waves: 6 fragment reads per 5 MFMAs)
    {44, IG_PIPE, 128, 128, 5, 4, 8, 0, 0.0},    // 5-slot ring = all 160 KiB of LDS: 4 tiles in flight
    {45, IG_PIPE, 96, 128, 5, 3, 6, 0, 1.0},     // 6 waves (3 x 2), 96-row tile: M = 2048 x N = 1280 -> 220 workgroups
    {46, IG_PIPE, 96, 128, 4, 3, 6, 0, 0.0},
    // 45 with ONE rendezvous per two k-tiles (S2).  Alone, on L2-resident operands, 2 - 4 % faster on every shape of the step; inside
    // the step, where the weights stream in cold, the tile less in flight costs more than the rendezvous saved: GEMM class 20.95 -
    // 21.04 vs 20.76 - 20.82 ms on one box (profiles/r03_two_tiles_per_rendezvous.txt).  Kept as the A/B partner, not selected.
    {47, IG_PIPE, 96, 128, 5, 3, 6, 1, 0.0},
    {49, IG_PIPE, 128, 160, 3, 4, 4, 0, 1.15},   // 4 waves 4x1 (32x160 wave tiles): N = 640 at 64^2 -> exactly 256 tiles
    {26, IG_WIDE, 256, 320, 3, 2, 8, 0, 1.05},   // 256x320, k-tile 32: linear GEGLU projections only
};
const Tile* find_tile(int number) {
  for (const Tile& t : kTiles) if (t.number == number) return &t;
  return nullptr;
}
const Tile& tile(int number) {
  if (const Tile* t = find_tile(number)) return *t;
  throw std::logic_error("igemm_select: no tile of that number");
}
// shapes a tile's kernel takes (wave tiles other than 64 columns leave no row statistics; the wide kernel is the GEGLU epilogue)
bool tile_takes(const Tile& t, const IgemmParams& p) {
  if (t.bn == 160) return p.N % 160 == 0 && !p.stat_out;
  if (t.bn == 320) return p.act == 1 && is_linear(p) && p.N % 320 == 0;
  return true;
}

// Cost of a grid of bm x bn tiles over an M x N output with nk k-tiles (arbitrary units, ~ns).  A workgroup's k-loop time goes
// with the bytes it stages per k-tile, (bm + bn) x 128 -- operand staging, not MFMA issue, bounds these kernels --
// and that holds per CU: a single round costs a full tile time however few CUs it fills (128x128 over 2048 x 1280 = 160
// workgroups takes as long per k-tile as 256 would).  Rounds after the first overlap with their predecessors' tails: a partly
// filled last round costs its fill fraction, but never less than 2/3.  FIXED ~ 8 us of launch / prologue / epilogue per round.
// w = 1.2 for the 8x1-wave 256x160 tile (6 fragment reads per 5 MFMAs), 1.05 for 256x320.
double tile_cost(int M, int N, int nk, int bm, int bn, double w) {
  const long tiles = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  const long full = tiles / 256, rem = tiles % 256;
  const double frac = rem == 0 ? 0.0 : (full == 0 ? 1.0 : (rem / 256.0 > 2.0 / 3.0 ? rem / 256.0 : 2.0 / 3.0));
  return ((double)full + frac) * (bm + bn) * nk * w + (double)(full + (rem ? 1 : 0)) * 3000.0;
}
double tile_cost(const IgemmParams& p, int nk, int number) {
  const Tile& t = tile(number);
  return tile_cost(p.M, p.N, nk, t.bm, t.bn, t.w);
}

// Tile choice by a two-term cost model fitted to the sweeps (profiles/r01_igemm_sweep.txt, r02_tile_sweep_256x160_256x320.txt,
// r02_tile_96x128.txt) -- tile_cost() above.  What the model buys: N = 320 / 1280 convs at 128^2 / 64^2 get 256x160 tiles =
// exactly one round (conv128 320: 95 -> 69 us, conv64 1280up: 353 -> 235 us), the GEGLU projections the one-round 256x320 tile
// (lin64 geglu 88 -> 77 us, lin32 geglu 67 -> 63 us), and the M = 2048 x N = 1280 linears (attention out / query projections,
// FF-out: 240 launches per step) 96x128 tiles -- 220 workgroups that each stage 12.5 % fewer bytes than the 160 of 128x128
// (19 -> 17 us, 54 -> 47 us), and the M = 8192 x N = 640 shapes of the 64^2 level 128x160 tiles (4 waves, 32x160 wave tiles) = exactly
// 256 workgroups where 256x128 made 160 (conv64 640 82 -> 70 us, 1920>640 243 -> 201, lin64 ff 44 -> 39; profiles/r02_tile_128x160.txt).
// `among`: the candidate numbers in the order that breaks ties.  Returns the tile's number.
int pick_tile(const IgemmParams& p, std::initializer_list<int> among) {
  const int nk = p.Kpad / 64;
  double best = 1e300;
  int number = 35;
  for (int n : among) {
    const Tile& t = tile(n);
    if (!tile_takes(t, p) || (n == 49 && p.act != 0)) continue;
    const double cost = tile_cost(p.M, p.N, nk, t.bm, t.bn, t.w);
    if (cost < best) { best = cost; number = n; }
  }
  if (number == 36 && nk >= 40) number = 44;   // long contractions: the 5-slot ring (4 tiles in flight) is 3-6 % faster (profiles/r02_ring5_ab.txt)
  return number;
}

// Phase form of an upsample convolution (IgemmParams::ph_rows): four 2x2-tap convolutions in one launch, a row tile inside one phase.
// The folded weights are rounded once more than the 3x3 ones, so WHETHER a layer runs folded changes bits: the rule looks at one entry
// (rows per entry and phase a multiple of 128: the 128-row tiles then fit any batch) and at nothing the batch changes.  Which of the fitting
// tiles runs changes no bit (same k order in all of them): tile_cost on the folded shape among the tiles whose rows divide a phase.
bool phase_shape_ok(const IgemmParams& p, int kt) {
  if (p.ph_rows <= 0 || p.ph_wbytes == 0 || p.B <= 0 || p.ph_rows != p.B * p.Hin * p.Win || p.M != 4 * p.ph_rows) return false;
  if (p.ksize != 2 || p.stride != 1 || p.up != 0 || p.pad != 1 || p.Hout != p.Hin || p.Wout != p.Win) return false;
  if ((p.Hin * p.Win) % 128 != 0 || p.Cin % kt != 0 || p.K != 4 * p.Cin || p.Kpad != p.K) return false;
  return p.act == 0 && p.n_split >= p.N && !p.R && !p.ebias && !p.stat_out && !p.gn_part && !p.ln_stat && !p.xa_k && !p.shadow;
}
int pick_phase_tile(const IgemmParams& p, int nk, bool hl) {
  double best = 1e300;
  int number = 36;
  for (int n : {35, 36, 38, 49}) {
    const Tile& t = tile(n);
    if (p.ph_rows % t.bm != 0 || !tile_takes(t, p) || (hl && n == 38)) continue;      // (no split-operand 256x160 instantiation)
    const double cost = tile_cost(p.M, p.N, nk, t.bm, t.bn, t.w);
    if (cost < best) { best = cost; number = n; }
  }
  if (!hl && number == 36 && nk >= 40) number = 44;      // as pick_tile
  return number;
}

// chip fill of the single-precision-class engines' 128-wide tiles: the f32 MFMA runs at 1/16 of the f16 rate and the split-operand
// product takes three, so those launches are matrix-pipe bound and the tile choice only has to keep the rounds of 256 CUs full
struct Fill { long t96, t128, t256; double eff128, eff256; };
Fill chip_fill(const IgemmParams& p) {
  const long cols = (p.N + 127) / 128;
  const long t96 = (long)((p.M + 95) / 96) * cols, t128 = (long)((p.M + 127) / 128) * cols, t256 = (long)((p.M + 255) / 256) * cols;
  return {t96, t128, t256, (double)t128 / (double)(((t128 + 255) / 256) * 256), (double)t256 / (double)(((t256 + 255) / 256) * 256)};
}
int fill_tile_256_or_128(const IgemmParams& p) {
  const Fill f = chip_fill(p);
  return f.eff256 >= f.eff128 ? 35 : 36;
}

// the grid of the CFG pair (2 entries of rpb rows) in 96-row tiles is at most two tiles per CU.  Where the weights-in-registers kernel
// pays (profiles/r04_wreg_first_ab.txt, r04_wreg_ab_l2.txt): with the shallow prefetch (L = 2: 72 KiB of LDS) two workgroups share a
// CU, so the 64^2 level's 430 tiles are one resident round (out-projection 19.5 -> 16.9 us, FF-out 44.5 -> 41.6 us, 1920 -> 640 skip
// 36.1 -> 33.1 us, cold weights) like the 32^2 level's 220 (18.2 -> 15.0, 47.8 -> 41.2 us).  Evaluated on the PAIR's shape whatever the
// actual batch: the two structures sum k in different orders.
bool wreg_pair_grid_fits(const IgemmParams& p) {
  const long rows = 2L * (p.rpb > 0 ? p.rpb : p.M);
  return ((rows + 95) / 96) * (long)(p.N / 128) <= 512;
}
// rows per weights-in-registers tile: 64 where that is still a single round of one tile per CU (small M: 512^2 images, single
// entries), else 96 -- the k-summation order does not depend on it.  (A 128-row tile -- 64 accumulators + 4 weight stages + 2 x 4
// fragments -- spilled fragment registers that were still in flight and was 30 - 75 % slower than the 96-row tile on every shape of
// the step: removed, profiles/r04_wreg_first_ab.txt.)
int wreg_rows(const IgemmParams& p) { return (long)((p.M + 63) / 64) * (p.N / 128) <= 256 ? 64 : 96; }
// shapes the weights-in-registers kernel takes: plain f16 linear layers / 1x1 convolutions whose weights were also packed in
// fragment order; `xa`: its XA instantiation -- the epilogue is the f16 cross-attention (with or without a folded LayerNorm in
// front) and nothing else
bool wreg_takes(const IgemmParams& p, const SelectKnobs& k, bool xa) {
  if (!p.Wf || !k.zero_page || (xa ? !p.xa_k || p.xa_k_lo : p.xa_k != nullptr)) return false;
  if (p.a_dt != DT_F16 || (p.c_dt != DT_F16 && (xa || p.c_dt != DT_F32))) return false;
  if (p.ksize != 1 || p.stride != 1 || p.up != 0 || p.pad != 0 || p.Hin != p.Hout || p.Win != p.Wout) return false;
  if (p.N % 128 != 0 || p.Cin != p.K || p.K != p.Kpad || p.Kpad % 64 != 0 || p.Kpad < 128) return false;
  if (p.act != 0 || p.n_split < p.N || p.gn_part || p.acc_scale || p.ebias) return false;
  if ((p.lda & 7) != 0 || misaligned16(p.A) || (p.ldc & 7) != 0 || misaligned16(p.C)) return false;
  if (xa) {
    if (p.stat_out || p.R || p.shadow || p.rpb <= 0 || p.rpb % 64 != 0 || p.M % p.rpb != 0 || p.xa_nctx < 1) return false;
    // more than one 96-key block (xattn_unit_long): the rule the plan asked before it packed the blocked image -- one predicate for both
    return p.xa_nctx <= 96 || igemm_xattn_ok(p.a_dt, p.c_dt, p.M, p.N, p.K, p.rpb, p.xa_nctx, k, true);
  }
  if (p.ln_stat || (p.R && ((p.ldr & 7) != 0 || misaligned16(p.R)))) return false;
  // f16 shadow of an fp32 output (+ the fp32 rows' statistics): whole 16-byte pieces
  if (p.shadow && (p.c_dt != DT_F32 || !p.shadow_gamma || (p.shadow_ld & (p.shadow_lo_scale < 0.f ? 15 : 7)) != 0 || misaligned16(p.shadow))) return false;
  return true;
}
#ifdef SDXL_MEASURE
// measure builds: forced weights-in-registers variants -- prefetch-depth A/B partners (68, 69; L = 2 in production), the 128-row tile
// (61), knock-out timing modes of the 96-row kernel (63 - 67: garbage results except 67; 70 - 72 per-stream: weights only /
// activations only / contiguous activations; 73 - 77: fetch stream + LDS reads, every byte an L2 hit / without the LDS reads / and
// without the rendezvous / fetch stream alone, real pointers / MFMAs + fetch stream, no LDS reads)
struct WregForced { int number, bm, depth, mode; };
constexpr WregForced kWregForced[] = {{61, 128, 2, 0}, {63, 96, 2, 1}, {64, 96, 2, 2}, {65, 96, 2, 3}, {66, 96, 2, 4}, {67, 96, 2, 5}, {68, 96, 3, 0},
    {69, 96, 4, 0}, {70, 96, 2, 6}, {71, 96, 2, 7}, {72, 96, 2, 8}, {73, 96, 2, 16 | 32}, {74, 96, 2, 16 | 32 | 4096}, {75, 96, 2, 16 | 32 | 4096 | 128},
    {76, 96, 2, 16 | 4096}, {77, 96, 2, 4096}};
#endif

void set_geometry(IgemmChoice& c, const IgemmParams& p) {
  const int tilesM = (p.M + c.bm - 1) / c.bm, tilesN = (p.N + c.bn - 1) / c.bn;
  c.grid = tilesM * tilesN * (c.splitk > 1 ? c.splitk : 1);
  switch (c.family) {
    case IG_GLDS: c.block = 256; c.lds = c.ns * (c.bm + c.bn) * 128; break;
    case IG_PIPE: {      // ring + LayerNorm coefficients where they still fit the 160 KiB
      const int ring = c.ns * (c.bm + c.bn) * 128;
      c.block = 64 * c.nw; c.lds = ring + 2048 <= 163840 ? ring + 2048 : ring;
    } break;
    // three slots (was four): the k-loop is not latency-bound and the whole ring is requested before the first MFMA -- 108 instead of
    // 144 KiB per CU; same-box library A/B on the bench line 21.19 / 21.12 -> 21.07 / 21.09 ms per step (profiles/r04_ring_depth_lib_ab.txt)
    case IG_WIDE: c.block = 512; c.lds = c.ns * (c.bm + c.bn) * 64 + 2048; break;
    case IG_WREG: {
      // warming workgroups: the CU slots the tile grid leaves empty in its (single) round -- one workgroup per CU up to 256 tiles, two up
      // to 512 -- at most 64 (a warmer pulls ~30 GB/s out of HBM: 36 of them move 13 MB inside an out-projection's 15 us)
      int warm = 0;
      if (p.warm[0] && p.warm_bytes[0] && c.grid <= 512) {
        const int spare = (c.grid <= 256 ? 256 : 512) - c.grid;
        warm = spare < 8 ? 0 : spare > 64 ? 64 : spare;
      }
      c.grid += warm;
      c.block = 512; c.lds = 2 * (c.ns + 1) * c.bm * 128 + (c.xa ? c.bm * 8 : 0);      // (XA: + the tile's LayerNorm coefficients)
    } break;
    case IG_GENERIC: c.block = 256; c.lds = 2 * (c.bm + c.bn) * 128; break;
    default: break;
  }
}
IgemmChoice from_tile(int number, int elem, const IgemmParams& p) {
  const Tile& t = tile(number);
  IgemmChoice c{};
  c.family = t.family; c.bm = t.bm; c.bn = t.bn; c.ns = t.ns; c.wgm = t.wgm; c.nw = t.nw; c.s2 = t.s2; c.elem = elem; c.a_elem = elem; c.splitk = 1;
  set_geometry(c, p);
  return c;
}
IgemmChoice wreg_choice(int bm, int depth, int mode, bool xa, const IgemmParams& p) {
  IgemmChoice c{};
  c.family = IG_WREG; c.bm = bm; c.bn = 128; c.ns = depth; c.nw = 8; c.mode = mode; c.elem = c.a_elem = DT_F16; c.splitk = 1;
  c.xa = xa ? (p.xa_nctx + 95) / 96 : 0;      // the context's 96-key blocks: 1 = the form with the block in registers, 2 .. 4 = the long form
  set_geometry(c, p);
  return c;
}
// weights-in-registers launch for a forced number (60 / 62: 96 / 64 rows per tile; measure builds: kWregForced), else rows by the rule
IgemmChoice wreg_forced_or_auto(int v, bool xa, const IgemmParams& p) {
#ifdef SDXL_MEASURE
  if (!xa) for (const WregForced& f : kWregForced) if (f.number == v) return wreg_choice(f.bm, f.depth, f.mode, false, p);
#endif
  return wreg_choice(v == 60 ? 96 : v == 62 ? 64 : wreg_rows(p), 2, 0, xa, p);
}

// f16 operands on the direct-to-LDS kernels; false: the shape (or a forced number that refuses it) is not theirs
bool select_f16(const IgemmParams& p, int v, const SelectKnobs& k, IgemmChoice& c) {
  if (!k.zero_page) return false;
  if (p.act > 1) return false;   // GELU / QuickGELU epilogues (CLIP MLP, once per prompt) live in the generic kernel
  if (p.a_dt != DT_F16 || (p.Cin % 64) != 0 || (p.lda % 8) != 0 || (p.Kpad % 64) != 0) return false;
  if (misaligned16(p.A)) return false;
  if (p.n_split < p.N && (p.n_split & 3) != 0) return false;
  if (p.ebias && (p.ebias_ld & 3) != 0) return false;
  if (p.stat_out && (v == 2 || v == 5 || v == 19 || v == 38)) return false;   // wave tiles narrower / other than 64 columns
  // (the DMA reads weight rows up to the tile edge: Npad is a multiple of 128 for every packed weight, pack_* kernels)
  const bool was_auto = v == 0;
  const int nk = p.Kpad / 64;
  if (p.ph_rows) {      // phase form of an upsample convolution: pipe tiles only, forced numbers do not apply
    if (!phase_shape_ok(p, 64)) throw std::runtime_error("igemm: the phase form of an upsample convolution was given a launch it does not take");
    c = from_tile(pick_phase_tile(p, nk, false), DT_F16, p);
    return true;
  }
  if (p.xa_k) {
    // fused cross-attention: wave tiles of 64 columns only, chosen by the same cost model
    if (p.act != 0 || p.n_split < p.N || p.stat_out || p.R || p.ebias ||
        !igemm_xattn_ok(p.a_dt, p.c_dt, p.M, p.N, p.K, p.rpb, p.xa_nctx, k, p.Wf && !p.xa_k_lo))
      throw std::runtime_error("igemm: fused cross-attention needs a plain f16 projection (no residual / split outputs)");
    if (!p.xa_k_lo && p.c_dt != DT_F16) throw std::runtime_error("igemm: the f16 fused cross-attention writes f16 rows");
    const bool forced_pipe = xattn_forced_pipe(v);     // forced pipe tiles stay forced
    // (above 96 keys igemm_xattn_ok has just answered for the weights-in-registers form: the pipe epilogues hold one block)
    if (p.xa_nctx > 96 && (forced_pipe || !igemm_wreg_xattn_selected(p, k)))
      throw std::runtime_error("igemm: fused cross-attention over more than 96 keys needs the weights-in-registers kernel");
    if (p.xa_k_lo) {     // split precision: the one-MFMA-row tiles only (128x128 / 96x128)
      c = from_tile(pick_tile(p, {36, 45}) == 45 ? 45 : 36, DT_F16, p);
      c.xh = 1;
      if (c.bm == 96) c.ns = 3;
    } else if (!forced_pipe && igemm_wreg_xattn_selected(p, k)) {
      // the f16 form of a layer whose weights also exist in fragment order: the weights-in-registers kernel with the attention behind its
      // partial-sum exchange (igemm_wreg.hip, XA instantiation; static rule per layer, knob "wreg_xattn")
      c = wreg_forced_or_auto(v, true, p);
      return true;
    } else {
      c = from_tile(forced_pipe ? v : pick_tile(p, {35, 36, 45}), DT_F16, p);
      if (c.bm == 96) c.ns = 3;     // (three slots, was five: 21.47 -> 21.39 / 21.38 ms per step with three / four, profiles/r04_ring_depth_lib_ab.txt)
    }
    c.xa = 1;
    set_geometry(c, p);
    return true;
  }
  if (p.gn_part) {
    if (!igemm_gn_part_ok(p, k)) throw std::runtime_error("igemm: GroupNorm statistics requested from a shape the 256x128 epilogue does not take");
    v = 0;            // (a forced test variant must not drop the statistics)
  }
  // plain linear layers / 1x1 convs whose weights also exist in fragment order: the weights-in-registers kernel (igemm_wreg.hip).
  // The rule is static per layer (never the batch), so its k-summation order (even + odd k-tiles) is what such a layer always gets.
  if (p.shadow) {      // f16 shadow of an fp32 output: written by the weights-in-registers epilogue only (run_conv asks igemm_wreg_selected before it sets the field)
    if (!igemm_wreg_selected(p, k)) throw std::runtime_error("igemm: an f16 shadow output needs the weights-in-registers kernel");
    c = wreg_forced_or_auto(0, false, p);
    return true;
  }
  if (v == 0 ? igemm_wreg_selected(p, k) : (v >= 60 && v <= 77 && wreg_takes(p, k, false))) { c = wreg_forced_or_auto(v, false, p); return true; }
  if (v >= 60 && v <= 77) return false;
  if (v == 0 && igemm_splitk_slices(p) > 1) {
    // long contractions over a small output (FF-out and the 32^2 convs of the CFG pair: M = 2048, N = 1280 is 80 tiles of
    // 256x128 on 256 CUs): three k-slices per tile fill the chip with the tile shape that moves the fewest bytes per flop
    c = from_tile(35, DT_F16, p);
    c.splitk = igemm_splitk_slices(p);
    set_geometry(c, p);
    return true;
  }
  if (v == 0) v = p.gn_part ? 35 : pick_tile(p, {35, 36, 45, 38, 49, 26});
#ifdef SDXL_MEASURE
  if (was_auto && !k.igemm_unrolled) {   // A/B against the rolled loops (profiles/r01_igemm_unrolled_ab.txt)
    if (v == 35) v = 11; else if (v == 36) v = 13; else if (v == 38) v = 19;
  }
#else
  (void)was_auto;
#endif
  const Tile* t = find_tile(v);
  if (!t) {
#ifdef SDXL_MEASURE
    c = IgemmChoice{}; c.family = IG_MEASURE; c.measure = v; c.splitk = 1;   // A/B partners, measurement modes (igemm_measure.hip): it refuses what it does not know
    return true;
#else
    return false;
#endif
  }
  if (!tile_takes(*t, p)) return false;
  c = from_tile(v, DT_F16, p);
  // (the operand-swapped V^T epilogue writes f16 rows)
  if (v == 35 && p.n_split < p.N && k.igemm_tsw && p.c_dt == DT_F16) c.tsw = 1;
#ifdef SDXL_MEASURE
  if (c.family == IG_WIDE) c.db = k.wide_db != 0;     // register-double-buffered fragment reads: measure builds only
#endif
  return true;
}

// Strict-fp32 mode on the same direct-to-LDS pipeline (the VAE at the reference's precision, sample/main.rs:121,273, and the
// parity configuration of the UNet): fp32 operands staged as 128-byte rows of 32 k-values, four v_mfma_f32_32x32x2_f32 per
// fragment pair.  false: a shape the generic kernel must take.
bool select_f32(const IgemmParams& p, const SelectKnobs& k, IgemmChoice& c) {
  if (!k.zero_page) return false;
  if (p.act > 1 || p.ln_stat || p.stat_out) return false;
  if (p.a_dt != DT_F32 || (p.Cin % 32) != 0 || (p.lda % 4) != 0 || (p.Kpad % 32) != 0) return false;
  if (misaligned16(p.A)) return false;
  if (p.n_split < p.N && (p.n_split & 3) != 0) return false;
  if (p.ebias && (p.ebias_ld & 3) != 0) return false;
  c = from_tile(fill_tile_256_or_128(p), DT_F32, p);
  return true;
}

// Split-operand mode (DT_HL; igemm_common.h): HL16 operands on the same direct-to-LDS pipeline, 3 f16 MFMAs per 16-deep product.
// false: a shape outside the pipeline (none in the VAE: its Cin % 32 != 0 layers are packed fp32).
bool select_hl(const IgemmParams& p, const SelectKnobs& k, IgemmChoice& c) {
  if (!k.zero_page) return false;
  if (p.act > 1 || p.ln_stat || p.stat_out || p.xa_k) return false;
  if (p.a_dt != DT_HL || (p.Cin % 32) != 0 || (p.lda % 4) != 0 || (p.Kpad % 32) != 0) return false;
  if (p.gn_part && !igemm_gn_part_ok(p, k)) throw std::runtime_error("igemm: GroupNorm statistics requested from a split-operand shape the 256x128 split-K epilogue does not take");
  if (misaligned16(p.A)) return false;
  if (p.n_split < p.N && (p.n_split & 3) != 0) return false;
  if (p.c_dt == DT_HL) {
    // HL16 outputs are written as whole 8-column (8-key) pieces: plain outputs with aligned rows, a fully transposed one (the
    // VAE's V^T) whose batch entries are whole pieces, or a split at a multiple of 128 columns (the UNet's q | k | V^T: a wave
    // tile is then wholly on one side); ragged splits go out as fp32
    if (p.n_split < p.N && p.n_split != 0 && ((p.n_split & 127) != 0 || p.act != 0)) return false;
    const int nout = p.act == 1 ? (p.N >> 1) : p.N;
    if (p.n_split != 0 && ((nout & 7) != 0 || (p.ldc & 15) != 0 || misaligned16(p.C))) return false;
    if (p.n_split < p.N && ((p.ct_ld & 15) != 0 || (p.rpb & 7) != 0 || (p.M % 8) != 0 || misaligned16(p.Ct))) return false;
  }
  if (p.ebias && (p.ebias_ld & 3) != 0) return false;
  if (p.ph_rows) {      // phase form of an upsample convolution (fp32 or HL16 rows out)
    if (!phase_shape_ok(p, 32)) throw std::runtime_error("igemm: the phase form of an upsample convolution was given a launch it does not take");
    c = from_tile(pick_phase_tile(p, p.Kpad / 32, true), DT_HL, p);
    return true;
  }
  const int t96mode = k.hl_tile96;     // bit 0: linear layers / 1x1 only (default), bit 1: 3x3 convolutions too (measured -0.15 % on the mixed mode's step: not selected)
  const bool splitk = (t96mode & 16) && igemm_splitk_slices(p) > 1;
  const bool plain160 = p.N % 160 == 0 && p.n_split >= p.N && !p.stat_out && p.act == 0;
  // round 5: the 96-row tile of the f16 engine for the shapes where it fills more of the chip's single round -- the M = 2048 x N = 1280 linears of the
  // 32^2 level (out-projections, cross-attention query projection, FF-out: 220 workgroups instead of 160).  Same k order in every tile shape, so the
  // choice never changes a result bit (A/B knob: sdxl_debug_set "hl_tile96").
  // (never a shape the in-launch split-K below would take: split-K depends on ONE entry's shape, this tile choice on the batched M -- testing it first
  //  would give a K >= 10240 linear layer one summation order at B <= 2 and another at B >= 3)
  const Fill f = chip_fill(p);
  int number;
  if ((t96mode & 1) && (p.ksize == 1 || (t96mode & 2)) && p.n_split >= p.N && f.t128 < 256 && f.t96 <= 256 && f.t96 > f.t128 && f.eff256 < (double)f.t96 / 256.0 && !splitk) {
    number = 45;
  } else if (splitk) {
    // (a 256x160 HL tile for the N = 320 convolutions of the 128^2 level -- no 17 % of column padding -- spills DMA pointers inside its k-loop: scratch
    //  loads in the VM queue break the hand-counted vmcnt waits.  Not instantiated.)
    // long contractions over a small output (the K >= 10240 convolutions of the 32^2 level: 80 tiles of 256x128): three k-slices per tile combined inside the
    // launch, as in the f16 engine (igemm_splitk_slices: depends on one batch entry's shape only; slabs summed in slice order: bit-reproducible) -- 240
    // workgroups instead of the 160 of 128x128 tiles.  Mixed-mode step 41.18 / 41.22 -> 40.60 / 40.56 ms, A/B/A/B; F32_SPLIT forward 2.16e-6 (was 2.12e-6),
    // config-2 final latent 2.4e-4 (2.1e-4) from the oracle (profiles/r05_hl_tile160_ab.txt; knob hl_tile96 bit 4)
    number = 35;
  } else if ((t96mode & 4) && plain160 && p.N % 128 != 0) {
    // the 4-wave 128x160 tile (one wave per SIMD, up to 512 registers each) for layers whose width is a multiple of 160 but not of 128 -- the N = 320
    // convolutions of the 128^2 level: two exact column tiles instead of three 128-wide ones with 17 % of padding.  Mixed-mode step 44.58 / 44.36 ->
    // 44.11 / 44.02 ms, A/B/A/B, results bit-identical (profiles/r05_hl_tile160_ab.txt; knob hl_tile96 bit 2)
    number = 49;
  } else if ((t96mode & 8) && plain160 &&
             tile_cost(p, p.Kpad / 32, 49) < std::min(tile_cost(p, p.Kpad / 32, 35), tile_cost(p, p.Kpad / 32, 36))) {
    // ... and where it fills the chip's rounds better than the 128-wide tiles (cost model of the f16 selection, tile_cost): the M = 8192 x N = 640 shapes of
    // the 64^2 level are exactly 256 tiles of 128x160 where 256x128 makes 160 and 128x128 320.  Mixed-mode step 41.14 / 41.32 -> 40.46 / 40.49 ms, A/B/A/B, bit-identical
    // (profiles/r05_hl_tile160_ab.txt; knob hl_tile96 bit 3)
    number = 49;
  } else {
    number = fill_tile_256_or_128(p);
  }
  c = from_tile(number, DT_HL, p);
  if (splitk) { c.splitk = igemm_splitk_slices(p); set_geometry(c, p); }
  return true;
}

// the generic kernel: the block tile minimising (#waves of the grid over the chip) x (tile cost / relative efficiency)
IgemmChoice select_generic(const IgemmParams& p, int compute_dt) {
  struct Cand { int bm, bn; float eff; };
  const Cand cands[4] = {{128, 128, 1.0f}, {128, 64, 0.85f}, {64, 128, 0.85f}, {64, 64, 0.70f}};
  int best = 0; float best_cost = 1e30f;
  for (int i = 0; i < 4; ++i) {
    if (p.act == 1 && cands[i].bn < 64) continue;
    const long tiles = (long)((p.M + cands[i].bm - 1) / cands[i].bm) * ((p.N + cands[i].bn - 1) / cands[i].bn);
    const int slots = 256 * (cands[i].bm * cands[i].bn >= 128 * 128 ? 2 : 4);
    const long waves = (tiles + slots - 1) / slots;
    const float cost = (float)waves * cands[i].bm * cands[i].bn / cands[i].eff;
    if (cost < best_cost) { best_cost = cost; best = i; }
  }
  IgemmChoice c{};
  c.family = IG_GENERIC; c.bm = cands[best].bm; c.bn = cands[best].bn; c.ns = 2; c.wgm = 2; c.nw = 4; c.splitk = 1;
  c.elem = compute_dt == DT_F16 ? DT_F16 : DT_F32;
  c.a_elem = compute_dt == DT_F16 && p.a_dt == DT_F16 ? DT_F16 : DT_F32;
  set_geometry(c, p);
  return c;
}
}  // namespace

// Split-K rule.  Like every rule that changes the summation order, a function of one batch entry's shape.
int igemm_splitk_slices(const IgemmParams& p) {
  if (!p.splitk_ws || !p.splitk_cnt) return 1;
  if (p.act != 0 || p.n_split < p.N || p.ln_stat) return 1;
  const int nk = p.Kpad / 64;
  // measured (profiles/r02_splitk_sweep.txt): pays from K ~ 11520 (the 32^2 convs: +4 % at K = 11520, +22 % at K = 23040); at
  // K = 5120 (FF-out) the serial combine costs more than the 24 % fewer bytes moved buy (57 vs 44 us), so the bar is 160 k-tiles
  // (round 6: N up to 1536 -- the refiner's 32^2 / 16^2 levels were excluded by the base model's 1280 and ran their K = 13824 ... 27648 convolutions on 12 - 48
  //  workgroups; and EIGHT slices where an entry has one 256-row tile: the 16^2 level of the refiner / of a 512^2 base image streams 42 - 85 MB of weights through
  //  12 x 8 workgroups instead of 12 x 3 -- profiles/r06_refiner_shape_profile.txt)
  if (p.rpb <= 0 || p.rpb > 1024 || p.N > 1536 || nk < 160) return 1;
  return p.rpb <= 256 ? 8 : 3;
}
size_t igemm_splitk_ws_bytes(int batch, int rows_per_entry, int n_max) {
  if (n_max > 1536) n_max = 1536;          // wider outputs never split (igemm_splitk_slices)
  const long rows3 = (long)batch * (rows_per_entry < 1024 ? rows_per_entry : 1024), rows8 = (long)batch * (rows_per_entry < 256 ? rows_per_entry : 256);
  const size_t slabs3 = (size_t)((rows3 + 255) / 256) * 3, slabs8 = (size_t)((rows8 + 255) / 256) * 8;
  return (slabs3 > slabs8 ? slabs3 : slabs8) * (size_t)((n_max + 127) / 128) * 256 * 128 * 4;
}

// GroupNorm statistics from the producing GEMM's epilogue (IgemmParams::gn_part): taken by the 256x128 kernel (plain or split-K)
// when that is the tile the selection picks anyway, whole 256-row tiles inside one batch entry, plain epilogue.  f16 operands, or
// (round 6) the split-operand convolutions the in-launch split-K takes: its staged epilogue leaves the statistics of the fp32 rows.
bool igemm_gn_part_ok(const IgemmParams& p, const SelectKnobs& k) {
  const bool hl = p.a_dt == DT_HL;
  const int kt = hl ? 32 : 64;
  if (hl ? p.c_dt != DT_F32 : (p.a_dt != DT_F16 || p.c_dt != DT_F16)) return false;
  if ((p.Cin % kt) != 0 || (p.lda % (kt / 8)) != 0 || (p.Kpad % kt) != 0) return false;
  if (p.act != 0 || p.n_split < p.N || p.stat_out || p.ln_stat || p.xa_k) return false;
  if (p.M % 256 != 0 || p.rpb <= 0 || p.rpb % 256 != 0 || p.N % 64 != 0) return false;
  if (p.ebias && (p.ebias_ld & 3) != 0) return false;
  if (hl) return (p.ldc & 3) == 0 && !misaligned16(p.C) && (k.hl_tile96 & 16) && igemm_splitk_slices(p) > 1;
  if (igemm_splitk_slices(p) > 1) return true;
  // The statistics path rounds differently from the statistics kernel, so the tile preference is evaluated for the CFG pair
  // (2 entries), whatever the actual batch.
  IgemmParams q = p;
  q.M = 2 * p.rpb;
  if (pick_tile(q, {35, 36, 45, 38, 26}) != 35) return false;
  // 128x160 tiles cannot leave the statistics (32x160 wave tiles): keep 256x128 + statistics unless the other tile saves more than
  // the statistics launch it brings back (~13 us ~ 6000 cost units)
  const int nk = p.Kpad / 64;
  return p.N % 160 != 0 || tile_cost(q, nk, 35) - tile_cost(q, nk, 49) < 6000.0;
}

bool igemm_xattn_ok(int a_dt, int c_dt, int M, int N, int K, int rpb, int n_ctx, const SelectKnobs& k, bool wreg_form) {
  // (c_dt: f16 rows; HL16 rows for the split-precision form behind an fp32-class out-projection -- the row / staged epilogues store either)
  if (!(a_dt == DT_F16 && (c_dt == DT_F16 || c_dt == DT_HL) && M > 0 && N % 64 == 0 && K % 64 == 0 && rpb > 0 && rpb % 64 == 0 && M % rpb == 0 && n_ctx >= 1))
    return false;
  if (n_ctx <= 96) return true;      // one block: every epilogue form; neither the knobs nor the weights' forms are read
  // 97 .. 384 keys: only the weights-in-registers XA form walks blocks (xattn_unit_long).  Everything of wreg_takes / igemm_wreg_xattn_selected that a
  // shape, the knobs or the operands' forms decide is decided HERE, so that the plan (UNet::set_context packs the blocked image,
  // spatial_transformer sets xa_k) and the selection cannot disagree: 128-column tiles, whole k-tiles, f16 rows, the pair's grid in one round,
  // the two A/B knobs, no forced pipe tile.  xattn_long_max_blocks: the last block count the fused form is kept for.
  if (!wreg_form || n_ctx > 96 * xattn_long_max_blocks || c_dt != DT_F16 || N % 128 != 0 || K < 128) return false;
  if (!k.zero_page || !k.igemm_wreg || !k.wreg_xattn || k.igemm_variant < 0 || xattn_forced_pipe(k.igemm_variant)) return false;
  IgemmParams q{};
  q.M = M; q.N = N; q.rpb = rpb;
  return wreg_pair_grid_fits(q);
}
bool igemm_phase_ok(const IgemmParams& p, int compute_dt, const SelectKnobs& k) {
  if (k.igemm_variant < 0 || !phase_shape_ok(p, compute_dt == DT_HL ? 32 : 64)) return false;
  IgemmChoice c{};
  return compute_dt == DT_F16 ? select_f16(p, 0, k, c) : (compute_dt == DT_HL && select_hl(p, k, c));
}
bool igemm_wreg_selected(const IgemmParams& p, const SelectKnobs& k) { return wreg_takes(p, k, false) && k.igemm_wreg && wreg_pair_grid_fits(p); }
bool igemm_wreg_xattn_selected(const IgemmParams& p, const SelectKnobs& k) {
  return wreg_takes(p, k, true) && k.igemm_wreg && k.wreg_xattn && wreg_pair_grid_fits(p);
}

IgemmChoice igemm_select(const IgemmParams& p, int compute_dt, const SelectKnobs& k) {
  IgemmChoice c{};
  if (p.M <= 0 || p.N <= 0) return c;     // IG_NONE: nothing to launch
  const int v = k.igemm_variant;          // -1 generic kernel only, 0 auto, > 0 a forced number
  if (compute_dt == DT_F16 && v >= 0 && select_f16(p, v, k, c)) return c;
  if (compute_dt == DT_F16 && v > 0 && select_f16(p, 0, k, c)) return c;   // forced tile refused the shape
  if (p.ph_rows && compute_dt != DT_HL) throw std::runtime_error("the phase form of an upsample convolution needs the f16 / split-operand direct-to-LDS kernels (igemm_phase_ok)");
  if (p.shadow && compute_dt != DT_F16) throw std::runtime_error("an f16 shadow output needs an f16 GEMM (weights-in-registers kernel)");
  if (compute_dt == DT_F32 && v >= 0 && select_f32(p, k, c)) return c;
  if (compute_dt == DT_HL) {     // no generic twin: layers the HL pipeline cannot take are packed (and launched) as fp32 by the host
    if (select_hl(p, k, c)) return c;
    throw std::runtime_error("split-operand (DT_HL) GEMM: shape / alignment outside the direct-to-LDS pipeline");
  }
  if (p.xa_k) throw std::runtime_error("fused cross-attention needs the f16 direct-to-LDS kernels");
  if (p.shadow) throw std::runtime_error("an f16 shadow output needs the f16 weights-in-registers kernel");
  // the generic kernels never write the GroupNorm statistics: a caller that was promised them (run_conv tags the output
  // Act and the consumer skips its statistics pass) must not get uninitialised memory -- forced variants, unaligned A, no zero page
  if (p.gn_part) throw std::runtime_error("GroupNorm statistics from the epilogue (gn_part) need the f16 direct-to-LDS 256x128 kernel");
  if (p.ln_stat || p.stat_out)
    throw std::runtime_error("LayerNorm-folded GEMM (ln_stat / stat_out) needs the f16 direct-to-LDS kernels");
  return select_generic(p, compute_dt);
}

// ---------------------------------------------------------------------------------------------------------
// attention, head dim 64
int attention_xsplit_heads(int H) { return H - std::max(1, H * 4 / 5); }
size_t attention_xsplit_counters(int B, int H, int Nq) { return (size_t)B * attention_xsplit_heads(H) * ((Nq + 63) / 64) * 2; }
size_t attention_xsplit_ws_bytes(int B, int H, int Nq) { return attention_xsplit_counters(B, H, Nq) * 2 * (9 * 64 * 4 * sizeof(float)); }

#ifdef SDXL_MEASURE
// knock-out timings of the key-split body (tools/attn_knockout.py): forced number -> the kernel's KO bits
struct AttnKnockout { int number, ko; };
constexpr AttnKnockout kAttnKnockouts[] = {{11, 1}, {12, 2}, {13, 4}, {14, 8}, {15, 16}, {16, 1 | 4}, {17, 2 | 8}};
#endif

AttnChoice attn_select(const AttnParams& p, const SelectKnobs& k) {
  const int v = k.attn_variant;     // -1: generic kernel only, 0: auto, forced numbers below
  AttnChoice c{};
  c.mix = -1; c.block = 256; c.grid_y = 1;
  const int qb128 = (p.Nq + 127) / 128, qb64 = (p.Nq + 63) / 64;
  const bool aligned = ((p.ldq | p.ldk | p.vt_ld | p.ldo) & 7) == 0 &&
                       ((reinterpret_cast<uintptr_t>(p.Q) | reinterpret_cast<uintptr_t>(p.K) |
                         reinterpret_cast<uintptr_t>(p.Vt) | reinterpret_cast<uintptr_t>(p.O)) & 15) == 0;
  if (p.dt == DT_F16 && (v == 0 || (v >= 2 && v <= 17)) && k.zero_page && aligned && !p.mask) {
    // 3-slot ring = 48 KiB per block -> three blocks per CU: the 640 blocks of the 64^2 level run as ONE round (a 4-slot
    // ring admits two per CU, a second half-empty round: 147 us vs 126 us measured); variant 3 keeps the 4-slot ring for A/B
    c.lds = 3 * 2 * 64 * 128;
    // key-split kernel (64-query blocks, waves = query sub-tile x key half): where 128-query blocks leave fewer than two
    // waves per SIMD (self-attention at 32^2: 160 blocks per batch entry) and the keys are whole 64-key tiles.
    // Made on one batch entry's grid (query blocks x heads), never the batch.
    const bool ks_ok = (p.Nk % 64) == 0 && p.Nk >= 128;
    const bool ks_pick = ks_ok && (v == 6 || ((v == 0 || v == 9) && qb128 * p.H < 256));
    // mixed block sizes (attn_d64_mix_kernel): the first 4/5 of the heads in 128-query blocks, the rest in 64-query key-split
    // blocks -- two large + one small block per CU for the CFG pair at 64^2 (121 -> 107 us; alone 78 -> 64 us, two pairs 210 ->
    // 218 us: profiles/r03_attention_block_balance.txt).  Like the pick above a function of one batch entry's shape only.
    // Level 1 (64-query + 32-query key-quarter blocks for the 32^2 shapes) measured no gain (23.2 -> 23.3 us) and is not picked.
    // Forced: 7 = level 0, 8 = level 1; 9 = the automatic choice without mixing (A/B).
    if (ks_ok && v == 7) c.mix = 0;
    else if (ks_ok && v == 8) c.mix = 1;
    else if (ks_ok && v == 0 && !ks_pick && p.H % 5 == 0) c.mix = 0;
    // level 2 where the key-split kernel would run (cross-workgroup key halves): 1/5 of the heads run as two half-key blocks per 64
    // queries, so that the CFG pair at the 32^2 level is 512 whole + 256 half blocks = two whole and one half block on every CU (2.5
    // units of work each) instead of three blocks on one half of the CUs and two on the other.  Whole 128-key pairs of tiles, a
    // workspace from the caller, heads divisible 4 : 1
    else if (ks_pick && v == 0 && p.xws && p.xcnt && k.attn_xsplit && p.H % 5 == 0 && p.H >= 5 && (p.Nk % 128) == 0 && (p.Nq % 64) == 0) c.mix = 2;
    if (c.mix >= 0) {
      c.kernel = AT_MIX;
      c.big_heads = p.H >= 2 ? std::max(1, p.H * 4 / 5) : 0;
      const int ql = c.mix == 0 ? 128 : 64;
      const int nl = p.B * c.big_heads * ((p.Nq + ql - 1) / ql);
      const int nsm = c.mix == 2 ? p.B * (p.H - c.big_heads) * 2 * ((p.Nq + ql - 1) / ql) : p.B * (p.H - c.big_heads) * ((p.Nq + ql / 2 - 1) / (ql / 2));
      c.grid_x = nl + nsm;
      return c;
    }
    if (ks_pick) {
      // (round 4: a software-pipelined form of this body -- QK^T of tile t issued around the softmax of tile t - 1, K and V^T on
      // separate rings -- measured 24.9 vs 22.6 us at the 32^2 level and was removed again: with three blocks per CU the other waves
      // already fill the chain's gaps, and the second live score tile costs registers; profiles/r04_attention_swp_ab.txt)
      c.kernel = AT_KS; c.grid_x = qb64 * p.B * p.H;
      return c;
    }
    c.grid_x = qb128 * p.B * p.H;
#ifdef SDXL_MEASURE
    if (ks_ok) for (const AttnKnockout& o : kAttnKnockouts) if (o.number == v) { c.kernel = AT_KS; c.ko = o.ko; c.grid_x = qb64 * p.B * p.H; return c; }
    if (v == 3 && p.Nk > 128) { c.kernel = AT_V2; c.ns = 4; c.lds = 4 * 2 * 64 * 128; return c; }
#endif
    c.kernel = AT_V2; c.ns = 3;
    return c;
  }
  c.grid_x = qb128; c.grid_y = p.B * p.H;
  if (p.dt == DT_F16 && v >= 0 && k.zero_page && aligned) { c.kernel = AT_F16; c.lds = 4 * 64 * 128; return c; }
  c.kernel = AT_GENERIC; c.elem = p.dt == DT_F16 ? DT_F16 : DT_F32;
  c.lds = p.dt == DT_F16 ? 4 * 64 * 128 : 4 * 64 * 256;
  return c;
}

}  // namespace sdxl
