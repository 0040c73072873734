// Host driver of csrc/mdxc_pool_plan.h (tests/test_host_mdxc_batch.py).
//   mdxc_pool_host tfc <hop> <dim_t> <overlap> <max_batch> {<n_samples>} x songs
//   mdxc_pool_host rof <hop> <dim_t> <step>    <max_batch> {<n_samples>} x songs
//   mdxc_pool_host fold <hop> <dim_t> <step> <n_samples>
// tfc / rof print "plan <chunk_size> <step> <front> <total> <per_pass>", per song "song <chunk0> <n_chunks> <pad> <padded_len>"
// (rof: pad and padded_len 0) and, rof only, "starts <start> ...", then per pass "pass <j0> <B>"; a rejected pool prints
// "error <message>" and exits with 3.  fold prints, per sample of one Roformer song, "<k_lo> <k_hi> <r_lo> <r_hi>": the chunk
// ranges roformer_finalize_pool_kernel walks (rof_fold_range).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../python-audio-separator_amd/csrc/mdxc_pool_plan.h"

int main(int argc, char **argv) {
  if (argc < 6) return 1;
  const int hop = atoi(argv[2]), dim_t = atoi(argv[3]);
  if (!strcmp(argv[1], "fold")) {
    const int64_t step = atoll(argv[4]), N = atoll(argv[5]), C = (int64_t)hop * (dim_t - 1);
    std::vector<int64_t> starts;
    const std::string why = rof_plan_starts(N, C, step, starts);
    if (!why.empty()) {
      printf("error %s\n", why.c_str());
      return 3;
    }
    for (int64_t i = 0; i < N; ++i) {
      const RofFoldRange r = rof_fold_range(i, N, C, step, (int64_t)starts.size());
      printf("%lld %lld %lld %lld\n", (long long)r.k_lo, (long long)r.k_hi, (long long)r.r_lo, (long long)r.r_hi);
    }
    return 0;
  }
  const bool rof = !strcmp(argv[1], "rof");
  const int max_batch = atoi(argv[5]);
  std::vector<int64_t> Ns;
  for (int i = 6; i < argc; ++i) Ns.push_back(atoll(argv[i]));
  MdxcPoolPlan pp;
  std::string err;
  const bool ok = rof ? mdxc_pool_build_rof(hop, dim_t, atoll(argv[4]), Ns.data(), (int)Ns.size(), pp, err)
                      : mdxc_pool_build_tfc(hop, dim_t, atoi(argv[4]), Ns.data(), (int)Ns.size(), pp, err);
  if (!ok) {
    printf("error %s\n", err.c_str());
    return 3;
  }
  const int total = pp.total(), per = total ? mdxc_pool_per_pass(total, max_batch) : 0;
  printf("plan %lld %lld %lld %d %d\n", (long long)pp.chunk_size, (long long)pp.step, (long long)pp.front, total, per);
  for (size_t i = 0; i < Ns.size(); ++i) {
    printf("song %d %d %lld %lld\n", pp.chunk0[i], pp.chunk0[i + 1] - pp.chunk0[i], rof ? 0ll : (long long)pp.tfc[i].pad,
           rof ? 0ll : (long long)pp.tfc[i].padded_len);
    if (rof) {
      printf("starts");
      for (int64_t s : pp.starts[i]) printf(" %lld", (long long)s);
      printf("\n");
    }
  }
  for (int j0 = 0; j0 < total; j0 += per) printf("pass %d %d\n", j0, std::min(per, total - j0));
  return 0;
}
