// body of f3::stft3p_kernel / f3::stft3p_pool_kernel (kernels_fft3.h), between the braces; `a` is the kernel's Stft3Args
  extern __shared__ cplx lds3[];
  cplx *buf = lds3;
  float *ring = reinterpret_cast<float *>(lds3 + LDS_X);
  cplx *twBs = reinterpret_cast<cplx *>(ring + NFFT);
  const int g = blockIdx.x, ch = blockIdx.y, b = blockIdx.z;
  const int j = threadIdx.x;
  const int t0 = group_start(g, a.T, a.n_groups), t1 = group_start(g + 1, a.T, a.n_groups) - 1;   // inclusive
  const int64_t C = a.C;
  const float *src;
  int64_t cstart = 0;
  if (a.n_song >= 0) {
    src = a.wave + (int64_t)ch * a.n_song;
    cstart = a.chunk_start[b];
  } else {
    src = a.wave + ((int64_t)b * 2 + ch) * C;
  }
  // hop h of the padded chunk = chunk positions [h * hop - n_fft / 2, + hop); this thread's four samples of it
  auto hop4 = [&](int64_t h) -> float4 {
    const int64_t q0 = h * HOP - NH + 4 * j;
    const int64_t s0 = a.n_song >= 0 ? cstart + q0 - a.trim : q0;
    const bool inside = q0 >= 0 && q0 + 4 <= C && (a.n_song < 0 || (s0 >= 0 && s0 + 4 <= a.n_song));
    if (inside && (reinterpret_cast<uintptr_t>(src + s0) & 15) == 0) return *reinterpret_cast<const float4 *>(src + s0);
    float x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t q = q0 + i;
      if (q < 0) q = -q;
      if (q >= C) q = 2 * (C - 1) - q;
      if (a.n_song >= 0) {
        const int64_t p = cstart + q - a.trim;
        x[i] = (p >= 0 && p < a.n_song) ? src[p] : 0.0f;
      } else {
        x[i] = src[q];
      }
    }
    return make_float4(x[0], x[1], x[2], x[3]);
  };
  if (j < 16 * 12) twBs[j] = a.twB[j];
#pragma unroll 1
  for (int d = 0; d < HPF; ++d) reinterpret_cast<float4 *>(ring + ((t0 + d) % HPF) * HOP)[j] = hop4(t0 + d);
  const int jb = j < NB ? j : 0;
  cplx win[12], wC[16];
#pragma unroll
  for (int r = 0; r < 12; ++r) win[r] = reinterpret_cast<const cplx *>(a.window)[j + 256 * r];
#pragma unroll
  for (int r = 1; r < 16; ++r) wC[r] = a.twC[r * NB + jb];
  const cplx twj = a.tw[j];
  const int64_t bst = a.out_bstride ? a.out_bstride : (int64_t)4 * a.T * a.dim_f;
  float *re0 = a.spec + (int64_t)b * bst + (int64_t)(ch * 2) * a.T * a.dim_f;
  const int64_t plane = (int64_t)a.T * a.dim_f;
  __syncthreads();
  for (int t = t0; t <= t1; ++t) {
    float4 nx = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < t1) nx = hop4((int64_t)t + HPF);                    // the hop frame t + 1 adds
    cplx v[12];
    {
      const cplx *ring2 = reinterpret_cast<const cplx *>(ring);
      const int base = (t % HPF) * (HOP / 2) + j;
#pragma unroll
      for (int r = 0; r < 12; ++r) {
        int pos = base + 256 * r;
        pos = pos >= NH ? pos - NH : pos;
        v[r] = emul(ring2[pos], win[r]);
      }
    }
    pass_a<-1>(j, v, buf);
    __syncthreads();
    cplx c[16];
    if (j < NB) pass_b_load(j, buf, c);
    __syncthreads();
    if (j < NB) pass_b_store<-1>(j, c, buf, twBs);
    __syncthreads();
    if (j < NB) pass_c_load(j, buf, c);
    __syncthreads();
    if (j < NB) {
#pragma unroll
      for (int r = 1; r < 16; ++r) c[r] = cmul(c[r], wC[r]);
      dft16<-1>(c);
#pragma unroll
      for (int r = 0; r < 16; ++r) buf[j + NB * r] = c[r];
    }
    // hop t (the oldest of frame t) is dead since the barrier after pass A: its slot takes the new hop
    if (t < t1) reinterpret_cast<float4 *>(ring + (t % HPF) * HOP)[j] = nx;
    __syncthreads();
    float *re = re0 + (int64_t)t * a.dim_f;
    float *im = re + plane;
    cplx twl = twj;
    asm volatile("" : "+v"(twl));                           // the eleven products below are recomputed per frame, not kept in 22 registers
#pragma unroll
    for (int r = 0; r < 12; ++r) {
      constexpr float C24[12] = {1.f, 0.96592582628906828675f, 0.86602540378443864676f, 0.70710678118654752440f, 0.5f,
                                 0.25881904510252076235f, 0.f, -0.25881904510252076235f, -0.5f, -0.70710678118654752440f,
                                 -0.86602540378443864676f, -0.96592582628906828675f};
      constexpr float S24[12] = {0.f, 0.25881904510252076235f, 0.5f, 0.70710678118654752440f, 0.86602540378443864676f,
                                 0.96592582628906828675f, 1.f, 0.96592582628906828675f, 0.86602540378443864676f,
                                 0.70710678118654752440f, 0.5f, 0.25881904510252076235f};
      const int k = j + 256 * r;
      if (k >= a.dim_f) continue;
      cplx X = mk(0.f, 0.f);
      if (k >= a.zero_low) {
        const cplx wk = r == 0 ? twl : cmulc_k(twl, mk(C24[r], S24[r]));   // W6144^(j + 256 r) = W6144^j W24^r
        X = cscale(split_bin(k, buf, wk), a.sign);
      }
      re[k] = X.x;
      im[k] = X.y;
    }
    __syncthreads();                                    // frame t + 1's pass A rewrites the exchange buffer
  }
