// body of stft_kernel / stft_pool_kernel (kernels_fft.h), between the braces; `a` / `p` are the kernel's StftArgs / FftPlan
  extern __shared__ float2 lds[];
  float2 *bufA = lds;
  float2 *bufB = lds + p.nh;
  const int t = blockIdx.x, ch = blockIdx.y, b = blockIdx.z;
  const int half = p.nh;  // n_fft / 2
  const int64_t C = a.C;
  const float *src;
  int64_t cstart = 0;
  if (a.n_song >= 0) {
    src = a.wave + (int64_t)ch * a.n_song;
    cstart = a.chunk_start[b];
  } else {
    src = a.wave + ((int64_t)b * 2 + ch) * C;
  }
  // load + window; LDS float pairs (x[2m], x[2m+1]) are the packed complex input
  float *fa = reinterpret_cast<float *>(bufA);
  for (int e = threadIdx.x; e < p.n_fft; e += blockDim.x) {
    int64_t q = (int64_t)t * a.hop + e - half;
    if (q < 0) q = -q;
    if (q >= C) q = 2 * (C - 1) - q;
    float v;
    if (a.n_song >= 0) {
      const int64_t j = cstart + q - a.trim;  // index into the un-padded mix
      v = (j >= 0 && j < a.n_song) ? src[j] : 0.0f;
    } else {
      v = src[q];
    }
    fa[e] = v * a.window[e];
  }
  float2 *Z = fft_lds<-1>(bufA, bufB, p, a.tw);
  // split: X[k] = E + e^{-2 pi i k / n} * O,  E = (Z[k] + conj Z[Nh-k]) / 2,  O = -i (Z[k] - conj Z[Nh-k]) / 2
  const int nh = p.nh;
  for (int k = threadIdx.x; k < a.dim_f; k += blockDim.x) {
    float re = 0.f, im = 0.f;
    if (k >= a.zero_low) {
      const float2 zk = Z[k == nh ? 0 : k];
      float2 zc = Z[(k == 0 || k == nh) ? 0 : nh - k];
      zc.y = -zc.y;
      const float2 E = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
      const float2 D = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y));
      const float2 O = make_float2(D.y, -D.x);
      float2 w = (k == nh) ? make_float2(-1.f, 0.f) : a.tw[k];
      const float2 X = cadd(E, cmul(w, O));
      re = X.x * a.sign;
      im = X.y * a.sign;
    }
    if (a.tf_layout == 2) {
      // BS-Roformer: b t (f s c) -- frequency-major with the stereo channel interleaved (bs_roformer.py:455-459)
      reinterpret_cast<float2 *>(a.spec)[(((int64_t)b * a.T + t) * a.dim_f + k) * 2 + ch] = make_float2(re, im);
    } else if (a.tf_layout) {
      const int kb = a.subbands > 1 ? a.subbands : 1;
      const int fs = a.dim_f / kb;
      const int j = k / fs, fp = k - j * fs;
      const int64_t bst = a.out_bstride ? a.out_bstride : (int64_t)4 * a.T * a.dim_f;
      const int64_t base = (int64_t)b * bst + (((int64_t)(ch * 2) * kb + j) * a.T + t) * fs + fp;
      a.spec[base] = re;
      a.spec[base + (int64_t)kb * a.T * fs] = im;
    } else {
      const int64_t base = (((int64_t)b * 4 + ch * 2) * a.dim_f + k) * a.T + t;
      a.spec[base] = re;
      a.spec[base + (int64_t)a.dim_f * a.T] = im;
    }
  }
