// The host side of the FLAC decoder (asx_flac_decode_*; no HIP): which streams it takes, the sizes of its scratch, and the walk that
// picks the stream's frames out of the candidates the device decoded.  Included by asx.hip and, for the host tests, by
// tests/host/flac_chain_host.cpp and tools/flac_host_decode.cpp.
//
// The walk.  A stream has no index: the frame kernel decodes every position whose header checks out, and leaves per candidate a record
// {pos, end, blocksize, assignment, ok}.  The stream's frames are the chain from byte 0 of the audio part: the next link is the `ok`
// candidate whose pos is the current link's end.  The chain stops at the end of the data or where no such candidate exists (a damaged or
// cut frame, a trailing tag): what was decoded up to there is the result, as libsndfile returns it.  An `ok` candidate off the chain -- a
// whole valid frame spelt by the samples of a VERBATIM subframe, or bits whose CRCs agree by chance -- is dropped.  A frame's samples go to
// the running sum of the chain's block sizes; the number coded in its header is not used.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

constexpr int FLACDEC_MIN_BLOCK = 16;
constexpr int FLACDEC_MAX_BLOCK = 16384;
constexpr int64_t FLACDEC_MAX_BYTES = ((int64_t)1 << 31) - 1;

struct FlacDecPlan {
  int64_t max_candidates = 0;   // two headers are at least 5 bytes apart
  int64_t slot_bytes = 0;       // per candidate found: two channels of max_blocksize int32
  int64_t scratch_bytes = 0;    // the counter, the candidate list and the records at max_candidates (the slots come on top)
};

struct FlacDecRec {
  uint32_t pos, end;
  int32_t blocksize, assignment, ok;
};

struct FlacDecLink {
  int32_t index;                // of the candidate
  int64_t out;                  // its first sample in the output
};

struct FlacDecChain {
  std::vector<FlacDecLink> links;
  int64_t n_samples = 0, n_frames = 0, bytes_consumed = 0;
};

// empty string, or why the stream is refused
static inline std::string flac_dec_plan_make(int64_t audio_bytes, int channels, int bps, int max_blocksize, int max_framesize, FlacDecPlan &p) {
  char buf[200];
  if (audio_bytes < 1) return "empty input (no audio frames behind the metadata)";
  if (audio_bytes > FLACDEC_MAX_BYTES) return "more than 2^31 - 1 bytes of audio frames";
  if (channels < 1 || channels > 2) {
    snprintf(buf, sizeof buf, "%d channels (the decoder takes mono and stereo streams)", channels);
    return buf;
  }
  if (bps < 8 || bps > 24) {
    snprintf(buf, sizeof buf, "%d bits per sample (8 .. 24; float32 holds no more exactly)", bps);
    return buf;
  }
  if (max_blocksize < FLACDEC_MIN_BLOCK || max_blocksize > FLACDEC_MAX_BLOCK) {
    snprintf(buf, sizeof buf, "maximum block size %d outside %d .. %d", max_blocksize, FLACDEC_MIN_BLOCK, FLACDEC_MAX_BLOCK);
    return buf;
  }
  if (max_framesize < 0) return "negative maximum frame size";
  p.max_candidates = audio_bytes / 5 + 1;
  p.slot_bytes = (int64_t)2 * max_blocksize * 4;
  p.scratch_bytes = 16 + p.max_candidates * 4 + p.max_candidates * (int64_t)sizeof(FlacDecRec);
  return "";
}

static inline void flac_dec_chain(const FlacDecRec *recs, int64_t n, int64_t audio_bytes, FlacDecChain &chain) {
  chain = FlacDecChain();
  std::vector<int32_t> order;
  for (int64_t i = 0; i < n; ++i)
    if (recs[i].ok && recs[i].end > recs[i].pos && (int64_t)recs[i].end <= audio_bytes && recs[i].blocksize >= 1) order.push_back((int32_t)i);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return recs[a].pos < recs[b].pos; });
  int64_t cur = 0;
  while (cur < audio_bytes) {
    // the first candidate at `cur` (of two at one position, the one listed first)
    auto it = std::lower_bound(order.begin(), order.end(), cur, [&](int32_t a, int64_t v) { return (int64_t)recs[a].pos < v; });
    if (it == order.end() || (int64_t)recs[*it].pos != cur) break;
    chain.links.push_back({*it, chain.n_samples});
    chain.n_samples += recs[*it].blocksize;
    cur = recs[*it].end;
  }
  chain.n_frames = (int64_t)chain.links.size();
  chain.bytes_consumed = cur;
}
