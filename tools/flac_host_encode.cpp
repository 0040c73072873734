// The FLAC block encoder of csrc/kernels_flac.h compiled for the host (ASX_FLAC_HOST: the lanes of every phase run one after another), so
// that its integer arithmetic, bit packing and CRCs can be checked and run under a sanitizer without a GPU.
//   g++ -O2 -std=c++17 -DASX_FLAC_HOST tools/flac_host_encode.cpp -o flac_host_encode
//   flac_host_encode in.s16 out.frames out.sizes sample_rate bits_per_sample block_size [pcm32]
// in.s16: interleaved little-endian int16 stereo.  out.frames: the audio frames back to back.  out.sizes: one int32 per frame.
// With a seventh argument "pcm32" the input is interleaved little-endian int32 stereo holding samples of bits_per_sample real bits, and the
// encoder is the int32 form (asx_flac_encode_pcm_dev's: no wasted bits, the side channel one bit wider).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../python-audio-separator_amd/csrc/kernels_flac.h"

int main(int argc, char **argv) {
  const bool pcm32 = argc == 8 && std::string(argv[7]) == "pcm32";
  if (argc != 7 && !pcm32) {
    fprintf(stderr, "usage: %s in.s16 out.frames out.sizes sample_rate bits_per_sample block_size [pcm32]\n", argv[0]);
    return 2;
  }
  using namespace asx::flac;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> pcm;
  int32_t v;
  while (fread(&v, 4, 1, f) == 1) pcm.push_back(v);
  fclose(f);
  const int sr = atoi(argv[4]), bps = atoi(argv[5]), bs = atoi(argv[6]);
  if (pcm.empty() || (bps != 16 && bps != 24) || bs < MIN_BLOCK || bs > MAX_BLOCK || (pcm32 && pcm.size() % 2)) return 2;
  if (pcm32)
    for (int32_t x : pcm)
      if (x < -(1 << (bps - 1)) || x >= (1 << (bps - 1))) return 2;
  Stream P{};
  P.pcm = pcm.data();
  P.n = (int64_t)pcm.size() / (pcm32 ? 2 : 1);
  P.block_size = bs;
  P.bps = bps;
  sample_rate_code(sr, &P.sr_code, &P.sr_extra_bits, &P.sr_extra);
  P.stride = pcm32 ? frame_stride(bs, bps + 1) : frame_stride(bs);
  const int64_t nb = (P.n + bs - 1) / bs;
  std::vector<uint8_t> frames((size_t)nb * P.stride);
  std::vector<int32_t> sizes((size_t)nb);
  P.frames = frames.data();
  P.frame_bytes = sizes.data();
  std::vector<uint8_t> lds((size_t)LDS_BYTES + 16);
  unsigned char *base = lds.data() + ((16 - ((uintptr_t)lds.data() & 15)) & 15);
  for (int64_t b = 0; b < nb; ++b) {
    if (pcm32) encode_block<true>(P, b, base);
    else encode_block<false>(P, b, base);
  }
  FILE *o = fopen(argv[2], "wb"), *s = fopen(argv[3], "wb");
  if (!o || !s) return 2;
  for (int64_t b = 0; b < nb; ++b) {
    if (sizes[b] < 0 || sizes[b] > P.stride) return 3;
    fwrite(frames.data() + (size_t)b * P.stride, 1, (size_t)sizes[b], o);
  }
  fwrite(sizes.data(), 4, sizes.size(), s);
  fclose(o);
  fclose(s);
  return 0;
}
