// Stand-alone driver of the upsample weight fold (csrc/upsample_fold.h) for the sanitizer test: reads cout, cin and cout * cin * 9 floats from the file
// named on the command line, folds them into heap buffers of exactly the documented sizes, and writes the 16 * cout * cin results to the second file.
#include "../stable-diffusion-xl-burn_amd/csrc/upsample_fold.h"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int dims[2] = {0, 0};
  if (std::fread(dims, sizeof(int), 2, in) != 2 || dims[0] <= 0 || dims[1] <= 0) return 4;
  const size_t pairs = (size_t)dims[0] * (size_t)dims[1];
  std::vector<float> w(pairs * 9), out(pairs * 16);
  if (std::fread(w.data(), sizeof(float), w.size(), in) != w.size()) return 5;
  std::fclose(in);
  sdxl::fold_upsample_weights(w.data(), out.data(), (size_t)dims[0], (size_t)dims[1]);
  FILE* of = std::fopen(argv[2], "wb");
  if (!of) return 6;
  if (std::fwrite(out.data(), sizeof(float), out.size(), of) != out.size()) return 7;
  std::fclose(of);
  return 0;
}
