// Stand-alone driver of csrc/select.cpp for sanitizer builds (tests/test_cpu_select.py compiles both with -fsanitize=address,undefined):
// reads the binary case list the test wrote -- records of (sdxl_igemm_case | sdxl_attn_case, sdxl_select_knobs) -- and runs every case
// through the selection.  Prints the number of choices and of refusals.
#include "../stable-diffusion-xl-burn_amd/csrc/select_debug.h"
#include <cstdio>
#include <stdexcept>
#include <vector>

template <typename Case, typename F> static int drive(const char* path, F run) {
  struct Rec { Case c; sdxl_select_knobs k; };
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 1; }
  std::vector<Rec> recs;
  Rec r;
  while (std::fread(&r, sizeof r, 1, f) == 1) recs.push_back(r);
  std::fclose(f);
  long chosen = 0, refused = 0, sum = 0;
  for (const Rec& x : recs) {
    try { sum += run(x.c, sdxl::select_debug_knobs(x.k)); ++chosen; } catch (const std::runtime_error&) { ++refused; }
  }
  std::printf("%ld %ld %ld\n", chosen, refused, sum);
  return 0;
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int a = drive<sdxl_igemm_case>(argv[1], [](const sdxl_igemm_case& c, const sdxl::SelectKnobs& k) {
    const sdxl::IgemmParams p = sdxl::select_debug_igemm(c);
    return (long)sdxl::igemm_gn_part_ok(p, k) + sdxl::igemm_wreg_selected(p, k) + sdxl::igemm_wreg_xattn_selected(p, k) + sdxl::igemm_select(p, c.compute_dt, k).grid;
  });
  const int b = drive<sdxl_attn_case>(argv[2], [](const sdxl_attn_case& c, const sdxl::SelectKnobs& k) { return (long)sdxl::attn_select(sdxl::select_debug_attn(c), k).grid_x; });
  return a | b;
}
