// Host driver of csrc/v3_norm.h (tests/test_host_mdxc_variants.py).
//   v3_norm_host fold <c> <in.bin> <out.bin>   in: weight, bias, running_mean, running_var (float32 [c] each); out: scale, shift
//   v3_norm_host splits <B> <G> <len>          prints the slice count of the GroupNorm statistics pass
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../python-audio-separator_amd/csrc/v3_norm.h"

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "fold")) {
    const int c = atoi(argv[2]);
    std::vector<float> in((size_t)4 * c), out((size_t)2 * c);
    FILE *f = fopen(argv[3], "rb");
    if (!f || fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    v3_bn_fold(c, in.data(), in.data() + c, in.data() + 2 * c, in.data() + 3 * c, 1e-5, out.data(), out.data() + c);
    f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 3;
    fclose(f);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "splits")) {
    printf("%d\n", v3_gn_splits(atoi(argv[2]), atoi(argv[3]), atoll(argv[4])));
    return 0;
  }
  return 1;
}
