// body of f3::stft3_kernel / f3::stft3_pool_kernel (kernels_fft3.h), between the braces; `a` is the kernel's Stft3Args
  extern __shared__ cplx lds3[];
  cplx *buf = lds3;
  const int t = blockIdx.x, ch = blockIdx.y, b = blockIdx.z;
  const int j = threadIdx.x;
  const int64_t C = a.C;
  const float *src;
  int64_t cstart = 0;
  if (a.n_song >= 0) {
    src = a.wave + (int64_t)ch * a.n_song;
    cstart = a.chunk_start[b];
  } else {
    src = a.wave + ((int64_t)b * 2 + ch) * C;
  }
  // frame element e sits at chunk position q = t * hop + e - n_fft / 2 (torch.stft centre padding, reflected at the chunk
  // ends, stft.py:41); song mode maps chunk position q to mix[cstart + q - trim] or 0 (mdx_separator.py:329-366)
  const int64_t q0 = (int64_t)t * HOP - NH;
  const bool inside_chunk = q0 >= 0 && q0 + NFFT <= C;
  const int64_t s0 = a.n_song >= 0 ? cstart + q0 - a.trim : q0;
  const bool fast = inside_chunk && (a.n_song < 0 || (s0 >= 0 && s0 + NFFT <= a.n_song)) &&
                    ((reinterpret_cast<uintptr_t>(src + s0) & 7) == 0);
  cplx v[12];
  const cplx *w2 = reinterpret_cast<const cplx *>(a.window);
  if (fast) {
    const cplx *s2 = reinterpret_cast<const cplx *>(src + s0);
#pragma unroll
    for (int r = 0; r < 12; ++r) {
      v[r] = emul(s2[j + 256 * r], w2[j + 256 * r]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 12; ++r) {
      float xe[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int64_t q = q0 + 2 * (j + 256 * r) + h;
        if (q < 0) q = -q;
        if (q >= C) q = 2 * (C - 1) - q;
        if (a.n_song >= 0) {
          const int64_t i = cstart + q - a.trim;
          xe[h] = (i >= 0 && i < a.n_song) ? src[i] : 0.0f;
        } else {
          xe[h] = src[q];
        }
      }
      const cplx w = w2[j + 256 * r];
      v[r] = mk(xe[0] * w.x, xe[1] * w.y);
    }
  }
  cplx c[16];
  pass_a<-1>(j, v, buf);
  __syncthreads();
  if (j < NB) pass_b_load(j, buf, c);
  __syncthreads();
  if (j < NB) pass_b_store<-1>(j, c, buf, a.twB);
  __syncthreads();
  if (j < NB) pass_c_load(j, buf, c);
  __syncthreads();
  if (j < NB) {
    pass_c_compute<-1>(j, c, a.twC);
#pragma unroll
    for (int r = 0; r < 16; ++r) buf[j + NB * r] = c[r];
  }
  __syncthreads();
  const cplx *bufA = buf;
  const int64_t bst = a.out_bstride ? a.out_bstride : (int64_t)4 * a.T * a.dim_f;
  float *re = a.spec + (int64_t)b * bst + ((int64_t)(ch * 2) * a.T + t) * a.dim_f;
  float *im = re + (int64_t)a.T * a.dim_f;
#pragma unroll
  for (int r = 0; r < 12; ++r) {
    const int k = j + 256 * r;
    if (k >= a.dim_f) continue;
    cplx X = mk(0.f, 0.f);
    if (k >= a.zero_low) {
      X = cscale(split_bin(k, bufA, a.tw[k]), a.sign);
    }
    re[k] = X.x;
    im[k] = X.y;
  }
