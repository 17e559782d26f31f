// attn_rows_flash_body.h -- NO include guard: the statements of the causal flash attention of gpt_rows.hip, included into the body of
// attn_rows_flash_kernel (one sequence) and of attn_rows_flash_seq (one sequence of a packed pass).  In scope at the include: KVT, OT,
// AttnRowsArgs a, and the macro FLASH_Q0 = the first query row of the workgroup's 128-row tile within the sequence.  Kept as text and
// not as a __device__ function: behind a function parameter the compiler allocates the one-sequence kernel differently.
  __shared__ __attribute__((aligned(16))) float Ks[FR_KT * FR_KP];
  __shared__ __attribute__((aligned(16))) float Vs[FR_KT * HD];
  const int hh = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int qw0 = FLASH_Q0 + wave * 32;  // first row of this wave
  const KVT* kb = reinterpret_cast<const KVT*>(a.kcache) + (size_t)hh * a.smax * HD;
  const KVT* vb = reinterpret_cast<const KVT*>(a.vcache) + (size_t)hh * a.smax * HD;
  const int last_key = a.pos0 + a.T - 1;  // last cache row this pass has written

  float qr[HD / 2];  // Q[row l31][d = 8m + 4 lh + i] for k-step 4m + i, scaled by log2(e) / sqrt(64)
  {
    const int qi = min(qw0 + l31, a.T - 1);
    const float* qp = a.q + (size_t)qi * a.D + hh * HD + 4 * lh;
    const float qs = 0.125f * 1.4426950408889634f;
#pragma unroll
    for (int m = 0; m < HD / 8; ++m) {
      const float4 t = *reinterpret_cast<const float4*>(qp + 8 * m);
      qr[4 * m] = t.x * qs; qr[4 * m + 1] = t.y * qs; qr[4 * m + 2] = t.z * qs; qr[4 * m + 3] = t.w * qs;
    }
  }
  f32x16 ot[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[j][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const int lim = a.pos0 + qw0 + l31;             // last key this lane's row may see
  const int wave_lim = a.pos0 + min(qw0 + 31, a.T - 1);  // ... and any row of this wave
  const int wg_lim = a.pos0 + min(FLASH_Q0 + 127, a.T - 1);
  const int t_first = (a.valid_from / FR_KT) * FR_KT;

  for (int t0 = t_first; t0 <= wg_lim; t0 += FR_KT) {
    __syncthreads();
    {  // stage 64 keys x 64 dims of K and V, widened to fp32: each thread one quarter row of each
      const int key = threadIdx.x >> 2, c16 = (threadIdx.x & 3) * 16;
      // rows past the pass repeat its last one, rows before valid_from (left padding: never written, the cache holds whatever the
      // allocation held -- 0 x NaN in the P V product would poison the row) repeat the first valid one; both are masked below
      const int t = min(max(t0 + key, a.valid_from), last_key);
      float kv[16], vv[16];
      load_row16<KVT>(kb + (size_t)t * HD + c16, kv);
      load_row16<KVT>(vb + (size_t)t * HD + c16, vv);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(Ks + key * FR_KP + c16 + 4 * i) = make_float4(kv[4 * i], kv[4 * i + 1], kv[4 * i + 2], kv[4 * i + 3]);
        *reinterpret_cast<float4*>(Vs + key * HD + c16 + 4 * i) = make_float4(vv[4 * i], vv[4 * i + 1], vv[4 * i + 2], vv[4 * i + 3]);
      }
    }
    __syncthreads();
    if (t0 > wave_lim) continue;  // wave-uniform: nothing in this tile is visible to this wave's rows

    f32x16 st[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[j][r] = 0.f;
    const float* kp0 = Ks + l31 * FR_KP + 4 * lh;
    const float* kp1 = kp0 + 32 * FR_KP;
    float4 ka[2][2];
    ka[0][0] = *reinterpret_cast<const float4*>(kp0);
    ka[0][1] = *reinterpret_cast<const float4*>(kp1);
#pragma unroll
    for (int m = 0; m < HD / 8; ++m) {
      if (m + 1 < HD / 8) {
        ka[(m + 1) & 1][0] = *reinterpret_cast<const float4*>(kp0 + 8 * (m + 1));
        ka[(m + 1) & 1][1] = *reinterpret_cast<const float4*>(kp1 + 8 * (m + 1));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float4 kk4 = ka[m & 1][j];
        st[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk4.x, qr[4 * m], st[j], 0, 0, 0);
        st[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk4.y, qr[4 * m + 1], st[j], 0, 0, 0);
        st[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk4.z, qr[4 * m + 2], st[j], 0, 0, 0);
        st[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk4.w, qr[4 * m + 3], st[j], 0, 0, 0);
      }
    }
    // causal / left-padding mask (only the first and the diagonal tiles have masked keys)
    if (t0 < a.valid_from || t0 + FR_KT - 1 > a.pos0 + qw0) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = t0 + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (key < a.valid_from || key > lim) st[j][r] = -INFINITY;
        }
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, st[j][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    // (a tile may be all -inf for a lane -- behind its limit: alpha = 1, weights 0.  A left-padding row, t < valid_from,
    // sees no key at all: its maximum stays -inf and is replaced by 0 in the exponents, so it ends as a row of zeros,
    // finite like everything else that reaches the cache)
    const float mn = fmaxf(m_run, tmax);
    const float mref = (mn == -INFINITY) ? 0.f : mn;
    const float alpha = __builtin_amdgcn_exp2f(m_run - mref);
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pw = __builtin_amdgcn_exp2f(st[j][r] - mref);
        st[j][r] = pw;
        psum += pw;
      }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = mn;
    if (alpha != 1.0f) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[j][r] *= alpha;
    }
    const float* vp = Vs + (4 * lh) * HD + l31;
    float va[2][2];
    va[0][0] = vp[0];
    va[0][1] = vp[32];
#pragma unroll
    for (int s2 = 0; s2 < 32; ++s2) {
      const int j = s2 >> 4, r = s2 & 15;
      if (s2 + 1 < 32) {
        const int j1 = (s2 + 1) >> 4, r1 = (s2 + 1) & 15;
        const float* vrow = vp + (j1 * 32 + (r1 & 3) + 8 * (r1 >> 2)) * HD;
        va[(s2 + 1) & 1][0] = vrow[0];
        va[(s2 + 1) & 1][1] = vrow[32];
      }
      const float pv = st[j][r];
      ot[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[s2 & 1][0], pv, ot[0], 0, 0, 0);
      ot[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[s2 & 1][1], pv, ot[1], 0, 0, 0);
    }
  }
  const int qi = qw0 + l31;
  if (qi < a.T) {
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    OT* op = reinterpret_cast<OT*>(a.out) + (size_t)qi * a.D + hh * HD;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) store_kv(op + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, ot[j][r] * inv);
  }
