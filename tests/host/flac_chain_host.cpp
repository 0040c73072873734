// The chain walk and the plan of the FLAC decoder (csrc/flac_dec_plan.h) on the host, for tests/test_host_flac_chain.py.
//   flac_chain_host chain audio_bytes [pos end blocksize assignment ok]...   -> "n_samples n_frames bytes_consumed" and one "index out" per link
//   flac_chain_host plan audio_bytes channels bits max_blocksize max_framesize -> "max_candidates slot_bytes scratch_bytes", or exit 1 + the refusal
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../python-audio-separator_amd/csrc/flac_dec_plan.h"

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "chain") && (argc - 3) % 5 == 0) {
    std::vector<FlacDecRec> recs;
    for (int i = 3; i < argc; i += 5)
      recs.push_back(FlacDecRec{(uint32_t)atoll(argv[i]), (uint32_t)atoll(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4])});
    FlacDecChain chain;
    flac_dec_chain(recs.data(), (int64_t)recs.size(), atoll(argv[2]), chain);
    printf("%lld %lld %lld\n", (long long)chain.n_samples, (long long)chain.n_frames, (long long)chain.bytes_consumed);
    for (const FlacDecLink &l : chain.links) printf("%d %lld\n", l.index, (long long)l.out);
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "plan")) {
    FlacDecPlan p;
    const std::string why = flac_dec_plan_make(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), p);
    if (!why.empty()) {
      printf("%s\n", why.c_str());
      return 1;
    }
    printf("%lld %lld %lld\n", (long long)p.max_candidates, (long long)p.slot_bytes, (long long)p.scratch_bytes);
    return 0;
  }
  fprintf(stderr, "usage: %s chain audio_bytes [pos end blocksize assignment ok]... | plan audio_bytes channels bits max_blocksize max_framesize\n", argv[0]);
  return 2;
}
