// The FLAC decoder of csrc/kernels_flac_dec.h compiled for the host (ASX_FLAC_HOST: the lanes of every phase run one after another) with the
// chain walk of csrc/flac_dec_plan.h, so that its parsing of true frames, false candidates and damaged frames can run under a sanitizer
// without a GPU.  Every buffer is allocated at exactly the size the device gets, so a read or write past one is a report.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DASX_FLAC_HOST tools/flac_host_decode.cpp -o flac_host_decode
//   flac_host_decode jobs.txt
// jobs.txt, one stream per line: in.audio out.f32 sample_rate channels bits_per_sample max_blocksize max_framesize
// in.audio: the audio part of a stream.  out.f32: the planar float32 mix [2, n].  Per line it prints: n_samples n_frames bytes_consumed n_candidates.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../python-audio-separator_amd/csrc/flac_dec_plan.h"
#include "../python-audio-separator_amd/csrc/kernels_flac_dec.h"

using namespace asx::flacdec;

static int decode_one(const char *in, const char *out, const Info &I) {
  FILE *f = fopen(in, "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  FlacDecPlan plan;
  const std::string why = flac_dec_plan_make(size, I.channels, I.bps, I.max_blocksize, I.max_framesize, plan);
  if (!why.empty()) {
    fclose(f);
    fprintf(stderr, "%s: %s\n", in, why.c_str());
    return 2;
  }
  uint8_t *a = static_cast<uint8_t *>(malloc((size_t)size));     // malloc: 16-byte aligned, and exactly `size` bytes
  if (fread(a, 1, (size_t)size, f) != (size_t)size) return 2;
  fclose(f);
  const uint32_t nbytes = (uint32_t)size;

  std::vector<uint32_t> cand;
  for (int64_t pos = 0; pos < size; ++pos)
    if (sync_at(a, size, pos, I)) cand.push_back((uint32_t)pos);
  if ((int64_t)cand.size() > plan.max_candidates) return 3;
  const size_t nc = cand.size();
  int32_t *slots = static_cast<int32_t *>(malloc((nc ? nc : 1) * (size_t)plan.slot_bytes));
  std::vector<FlacDecRec> recs(nc);
  static_assert(sizeof(FlacDecRec) == REC_WORDS * 4, "record layout");
  unsigned char *lds = static_cast<unsigned char *>(malloc((size_t)lds_bytes(I.max_blocksize)));
  for (size_t c = 0; c < nc; ++c) decode_candidate(a, nbytes, I, cand.data(), (uint32_t)c, slots, reinterpret_cast<int32_t *>(recs.data()), lds);

  FlacDecChain chain;
  flac_dec_chain(recs.data(), (int64_t)nc, size, chain);
  const int64_t n = chain.n_samples;
  std::vector<float> mix((size_t)(2 * n));
  const float scale = 1.0f / (float)(1 << (I.bps - 1));
  for (const FlacDecLink &L : chain.links) {
    const FlacDecRec &r = recs[(size_t)L.index];
    const int32_t *s0 = slots + (int64_t)L.index * 2 * I.max_blocksize;
    const int32_t *s1 = I.channels == 2 ? s0 + I.max_blocksize : s0;
    for (int i = 0; i < r.blocksize; ++i) {
      int64_t l, rr;
      undo_stereo(r.assignment, (int64_t)s0[i], (int64_t)s1[i], l, rr);
      mix[(size_t)(L.out + i)] = (float)l * scale;
      mix[(size_t)(n + L.out + i)] = (float)rr * scale;
    }
  }
  FILE *o = fopen(out, "wb");
  if (!o) return 2;
  if (n) fwrite(mix.data(), 4, mix.size(), o);
  fclose(o);
  printf("%lld %lld %lld %zu\n", (long long)n, (long long)chain.n_frames, (long long)chain.bytes_consumed, nc);
  free(lds);
  free(slots);
  free(a);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s jobs.txt\n", argv[0]);
    return 2;
  }
  FILE *jobs = fopen(argv[1], "r");
  if (!jobs) return 2;
  char in[1024], out[1024];
  Info I{};
  while (fscanf(jobs, "%1023s %1023s %d %d %d %d %d", in, out, &I.sample_rate, &I.channels, &I.bps, &I.max_blocksize, &I.max_framesize) == 7) {
    const int rc = decode_one(in, out, I);
    if (rc) return rc;
  }
  fclose(jobs);
  return 0;
}
