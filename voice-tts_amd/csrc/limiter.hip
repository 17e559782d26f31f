// limiter.hip -- the peak side of the output stage's level control: the 4x-oversampled true peak of every hop of a programme
// (ITU-R BS.1770 Annex 2, a 49-tap Hann-windowed sinc), and a non-causal look-ahead limiter that holds a programme under its ceiling
// with a gain per sample.  Programmes are described by the row tables of output.hip ((src, n, dst) triples, zeros in the gaps);
// nothing is allocated here, and there is no floating-point atomic: a programme's numbers are the same alone and in any launch.
//
// Interpolator.  h[m] = sinc(m / 4) 0.5 (1 + cos(pi m / 24)), m = -24 .. 24 (fp64, from the host).  The point n + k / 4 of a
// programme y is z[4 n + k] = sum_j h[k - 4 j] y[n + j]; k = 0 is the sample itself, and for k = 1 .. 3 the taps that exist are
// j = -5 .. 6, twelve per phase (h[+-24] = 0).  fp64, ascending j, over the fp32 samples.
#include "common.h"

namespace ixtts {

constexpr int TP_THREADS = 256;
constexpr int TP_LO = 5, TP_PHASE_TAPS = 12;  // y[n - 5 .. n + 6]
constexpr int TP_MAX_HOP = IXTTS_LOUDNESS_MAX_HOP;
constexpr int LIM_TILE = IXTTS_LIMITER_TILE;
constexpr int LIM_THREADS = 256;
constexpr int LIM_MAX_W = IXTTS_LIMITER_MAX_W;
constexpr int LIM_HALO = 7;  // samples of y beyond the detector's range (the interpolator reaches 6)
constexpr int LIM_R = LIM_TILE + 4 * LIM_MAX_W;
static_assert(LIM_TILE % LIM_THREADS == 0, "every thread owns LIM_TILE / LIM_THREADS samples of a tile");
constexpr int LIM_OWN = LIM_TILE / LIM_THREADS;

// The programme's samples [p0, p0 + len) (counted from its start) times g into w: the rows that reach into the range, copied
// coalesced; zeros in the gaps, before the start and behind the end.  (g = 1 leaves a sample as it is.)
__device__ __forceinline__ void stage_programme(float* w, int len, long long p0, const float* __restrict__ x, long x_elems, const long long* __restrict__ rows,
                                                long long row_lo, long long nr, long long start, long long extent, float g, int tid, int threads) {
  for (int i = tid; i < len; i += threads) w[i] = 0.0f;
  __syncthreads();
  const long long w0 = start + p0, w1 = min(start + p0 + len, start + extent);
  for (long long r = row_lo; r < row_lo + nr; ++r) {
    const long long src = rows[3 * r], n = rows[3 * r + 1], dst = rows[3 * r + 2];
    const long long a = max(max(dst, w0), start), b = min(dst + n, w1);
    if (n <= 0 || a >= b || src < 0 || src + n > x_elems) continue;  // (a source outside the input reads as silence)
    const float* xs = x + src + (a - dst);
    float* ws = w + (a - w0);
    const int m = (int)(b - a);
    for (int i = tid; i < m; i += threads) ws[i] = __fmul_rn(g, xs[i]);
  }
  __syncthreads();
}

// the three phases' taps as the kernels read them: ph[k - 1][jj] = h[k - 4 (jj - 5)]
__device__ __forceinline__ void stage_phases(double (*ph)[TP_PHASE_TAPS], const double* __restrict__ taps, int tid) {
  if (tid < 3 * TP_PHASE_TAPS) {
    const int k = tid / TP_PHASE_TAPS + 1, jj = tid % TP_PHASE_TAPS;
    ph[k - 1][jj] = taps[(k - 4 * (jj - TP_LO)) + 24];
  }
}

// max |z| over the three inter-sample points behind the sample whose y[n - 5] is w[0]
__device__ __forceinline__ double intersample_max(const double (*ph)[TP_PHASE_TAPS], const float* w) {
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double acc = 0.0;
#pragma unroll
    for (int jj = 0; jj < TP_PHASE_TAPS; ++jj) acc = fma(ph[k][jj], (double)w[jj], acc);
    q = fmax(q, fabs(acc));
  }
  return q;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// ------------------------------------------------------------------------------------------------------------------- true peak
// One workgroup per hop of a programme in true mode (`modes` null: every programme): the hop and the interpolator's halo in LDS, a
// thread takes samples at a stride -- the sample, three phases of twelve taps -- and the maximum of |.| goes to the hop's slot of the
// hop-peak array, rounded to fp32 once.  A maximum does not depend on its order.
__global__ __launch_bounds__(TP_THREADS) void true_peak_kernel(const float* __restrict__ x, long x_elems, const long long* __restrict__ rows, int n_rows,
                                                               const long long* __restrict__ reqs, const long long* __restrict__ modes,
                                                               const double* __restrict__ taps, float* __restrict__ hop_peak, long hops_elems) {
  __shared__ float w[TP_MAX_HOP + TP_PHASE_TAPS];  // programme [t0 - 5, t0 + valid + 6]
  __shared__ double ph[3][TP_PHASE_TAPS];
  __shared__ double part[TP_THREADS / 64];
  if (modes && modes[blockIdx.y] != 1) return;
  const long long* rq = reqs + (long)blockIdx.y * IXTTS_LOUDNESS_REQ_COLS;
  const long long row_lo = rq[0], nr = rq[1], start = rq[2], extent = rq[3], H64 = rq[4], slot = rq[5] + blockIdx.x;
  if (H64 <= 0 || H64 > TP_MAX_HOP || extent <= 0) return;
  const int H = (int)H64;
  const long long t0 = (long long)blockIdx.x * H;
  if (t0 >= extent) return;  // (the grid is cut for the programme with the most hops)
  if (slot < 0 || slot >= hops_elems || row_lo < 0 || nr < 0 || row_lo + nr > n_rows) return;
  const int tid = threadIdx.x;
  const int valid = (int)min((long long)H, extent - t0);
  stage_phases(ph, taps, tid);
  stage_programme(w, valid + TP_PHASE_TAPS - 1, t0 - TP_LO, x, x_elems, rows, row_lo, nr, start, extent, 1.0f, tid, TP_THREADS);
  double best = 0.0;
  for (int i = tid; i < valid; i += TP_THREADS) best = fmax(best, fmax(fabs((double)w[i + TP_LO]), intersample_max(ph, w + i)));
  best = wave_max_f64(best);
  if ((tid & 63) == 0) part[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < TP_THREADS / 64; ++k) best = fmax(best, part[k]);
    hop_peak[slot] = (float)best;
  }
}

// --------------------------------------------------------------------------------------------------------------------- limiter
// One workgroup per tile of LIM_TILE output samples of a limited programme, everything out of LDS (W = the look-around of the
// programme's rate, 5 ms; c = its ceiling in sample units; y = fp32(g x), g read from the gating kernel's array):
//   y  over [t0 - 2W - 7, t0 + T + 2W + 7)
//   p  the detector: |y[n]|, in true mode the max with |z| at the seven points from n - 3/4 to n + 3/4 (an inter-sample point is
//      charged to both of its neighbours; points exist for n in [0, N) only)
//   r  = min(1, c / p) over [t0 - 2W, t0 + T + 2W), 1 where p = 0 and outside [0, N)
//   m  = min over |k| <= W of r[n + k], over [t0 - W, t0 + T + W): minima over runs of 1, 2, 4 .. samples by doubling, the window
//      of 2W + 1 as the min of two overlapping runs (a minimum does not depend on its order)
//   a  = 1 - sum_k w[k] (1 - m[n - W + k]), k = 0 .. 2W ascending, w the normalised Hann window of the rate (fp64): every m in the
//      sum has n in its own window, so a <= r[n]; fp32(a) is stepped one ulp toward zero where rounding put it above r[n]
// and out[n] = fp32(a) * y[n], one rounding.  A tile whose r is 1 throughout copies y (the sum is exactly 0).  Per tile the smallest
// fp32(a) (as its bit pattern: the values are positive) and the number of samples with fp32(a) < 1 go to the tile's two words of
// `partials`; the host reduces them in tile order.
__global__ __launch_bounds__(LIM_THREADS) void limiter_kernel(const float* __restrict__ x, long x_elems, const long long* __restrict__ rows, int n_rows,
                                                              const long long* __restrict__ lreqs, const double* __restrict__ ceilings,
                                                              const double* __restrict__ tables, long tables_elems, const float* __restrict__ gains,
                                                              int n_gains, float* out, long out_elems, unsigned int* __restrict__ partials,
                                                              long partial_slots) {
  __shared__ float sy[LIM_R + 2 * LIM_HALO + 2];
  __shared__ double bufA[LIM_R + 2];
  __shared__ double bufB[LIM_R + 2];
  __shared__ double ph[3][TP_PHASE_TAPS];
  __shared__ unsigned int smin[LIM_THREADS / 64], scnt[LIM_THREADS / 64];
  const long long* lq = lreqs + (long)blockIdx.y * IXTTS_LIMITER_REQ_COLS;
  const long long row_lo = lq[0], nr = lq[1], start = lq[2], extent = lq[3], out_off = lq[4], gi = lq[5], W64 = lq[6], w_off = lq[7], mode = lq[8];
  const long long slot = lq[9] + blockIdx.x;
  const long long t0 = (long long)blockIdx.x * LIM_TILE;
  if (extent <= 0 || t0 >= extent) return;  // (the grid is cut for the longest programme)
  // a programme its buffers cannot hold is left alone: nothing is read or written outside them
  if (W64 < 1 || W64 > LIM_MAX_W || w_off < IXTTS_TRUE_PEAK_TAPS || w_off + 2 * W64 + 1 > tables_elems) return;
  if (out_off < 0 || out_off + extent > out_elems || slot < 0 || slot >= partial_slots || row_lo < 0 || nr < 0 || row_lo + nr > n_rows) return;
  const int tid = threadIdx.x;
  const int W = (int)W64, L = 2 * W + 1;
  const int tile = (int)min((long long)LIM_TILE, extent - t0);
  const int n_r = tile + 4 * W;  // r over [t0 - 2W, t0 + tile + 2W)
  const int n_m = tile + 2 * W;  // m over [t0 - W, t0 + tile + W)
  const double c = ceilings[blockIdx.y];
  const float g = (gi >= 0 && gi < n_gains) ? gains[gi] : 1.0f;
  stage_phases(ph, tables, tid);
  stage_programme(sy, n_r + 2 * LIM_HALO, t0 - 2 * W - LIM_HALO, x, x_elems, rows, row_lo, nr, start, extent, g, tid, LIM_THREADS);
  // bufA[i]: the largest |z| at the three points behind sample n = t0 - 2W - 1 + i; y[n - 5] = sy[i + 1]
  for (int i = tid; i < n_r + 1; i += LIM_THREADS) {
    const long long n = t0 - 2 * W - 1 + i;
    bufA[i] = (mode == 1 && n >= 0 && n < extent) ? intersample_max(ph, sy + i + 1) : 0.0;
  }
  __syncthreads();
  int any = 0;
  for (int i = tid; i < n_r; i += LIM_THREADS) {
    const long long n = t0 - 2 * W + i;
    double r = 1.0;
    if (n >= 0 && n < extent) {
      const double p = fmax(fmax(fabs((double)sy[i + LIM_HALO]), bufA[i + 1]), bufA[i]);
      if (p > c) r = c / p;
    }
    bufB[i] = r;
    any |= r < 1.0;
  }
  any = __syncthreads_or(any);
  unsigned int mn = 0x3f800000u, cnt = 0;  // fp32 1.0
  const float* ty = sy + 2 * W + LIM_HALO;  // y[t0]
  float* to = out + out_off + t0;
  if (!any) {
    for (int t = tid; t < tile; t += LIM_THREADS) to[t] = ty[t];
  } else {
    double own[LIM_OWN];  // r of the samples this thread writes
#pragma unroll
    for (int e = 0; e < LIM_OWN; ++e) own[e] = bufB[min(2 * W + tid + e * LIM_THREADS, n_r - 1)];
    double *cur = bufB, *nxt = bufA;
    int width = 1;  // cur[i] = min r[i .. i + width)
    while (2 * width <= L) {
      for (int i = tid; i < n_r; i += LIM_THREADS) nxt[i] = i + width < n_r ? fmin(cur[i], cur[i + width]) : cur[i];
      __syncthreads();
      double* s = cur; cur = nxt; nxt = s;
      width *= 2;
    }
    for (int i = tid; i < n_m; i += LIM_THREADS) nxt[i] = 1.0 - fmin(cur[i], cur[i + L - width]);  // 1 - m; i + L - 1 <= n_r - 1
    __syncthreads();
    const double* d = nxt + tid;  // (1 - m)[t0 - W + tid ..]
    const double* wt = tables + w_off;
    double s[LIM_OWN];
#pragma unroll
    for (int e = 0; e < LIM_OWN; ++e) s[e] = 0.0;
    if (tile == LIM_TILE) {
      for (int k = 0; k < L; ++k) {
        const double wk = wt[k];
#pragma unroll
        for (int e = 0; e < LIM_OWN; ++e) s[e] = fma(wk, d[e * LIM_THREADS + k], s[e]);
      }
    } else {
      for (int k = 0; k < L; ++k) {
        const double wk = wt[k];
#pragma unroll
        for (int e = 0; e < LIM_OWN; ++e)
          if (tid + e * LIM_THREADS < tile) s[e] = fma(wk, d[e * LIM_THREADS + k], s[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < LIM_OWN; ++e) {
      const int t = tid + e * LIM_THREADS;
      if (t >= tile) break;
      float a32 = (float)(1.0 - s[e]);
      if ((double)a32 > own[e] && a32 > 0.0f) a32 = __uint_as_float(__float_as_uint(a32) - 1u);
      to[t] = __fmul_rn(a32, ty[t]);
      cnt += a32 < 1.0f;
      mn = min(mn, __float_as_uint(a32));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = min(mn, (unsigned int)__shfl_xor((int)mn, o, 64));
    cnt += (unsigned int)__shfl_xor((int)cnt, o, 64);
  }
  if ((tid & 63) == 0) { smin[tid >> 6] = mn; scnt[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < LIM_THREADS / 64; ++k) { mn = min(mn, smin[k]); cnt += scnt[k]; }
    partials[2 * slot] = mn;
    partials[2 * slot + 1] = cnt;
  }
}

}  // namespace ixtts

using namespace ixtts;

extern "C" int ixtts_limiter_tile(void) { return LIM_TILE; }

extern "C" int ixtts_true_peak(const float* x_dev, long x_elems, const int64_t* rows_dev, int n_rows, const int64_t* reqs_dev, const int64_t* modes_dev,
                               int n_reqs, long max_hops, const double* taps_dev, float* hop_peak_dev, long hops_elems, void* stream) {
  IX_ARG(rows_dev && reqs_dev && taps_dev && hop_peak_dev && (x_dev || x_elems == 0), "true_peak: null pointer");
  IX_ARG(n_rows >= 0 && x_elems >= 0 && n_reqs >= 0 && n_reqs <= 65535 && max_hops >= 0 && max_hops <= 0x7fffffffL && hops_elems >= 0,
         "true_peak: bad shape n_rows=%d x_elems=%ld n_reqs=%d max_hops=%ld hops_elems=%ld", n_rows, x_elems, n_reqs, max_hops, hops_elems);
  if (n_reqs == 0 || max_hops == 0) return IXTTS_OK;
  hipLaunchKernelGGL(true_peak_kernel, dim3((unsigned)max_hops, (unsigned)n_reqs), dim3(TP_THREADS), 0, (hipStream_t)stream, x_dev, x_elems,
                     (const long long*)rows_dev, n_rows, (const long long*)reqs_dev, (const long long*)modes_dev, taps_dev, hop_peak_dev, hops_elems);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

extern "C" int ixtts_limiter(const float* x_dev, long x_elems, const int64_t* rows_dev, int n_rows, const int64_t* lreqs_dev, const double* ceilings_dev,
                             int n_reqs, long max_tiles, const double* tables_dev, long tables_elems, const float* gains_dev, int n_gains, float* out_dev,
                             long out_elems, uint32_t* partials_dev, long partial_slots, void* stream) {
  IX_ARG(rows_dev && lreqs_dev && ceilings_dev && tables_dev && out_dev && partials_dev && (x_dev || x_elems == 0) && (gains_dev || n_gains == 0),
         "limiter: null pointer");
  IX_ARG(n_rows >= 0 && x_elems >= 0 && n_reqs >= 0 && n_reqs <= 65535 && max_tiles >= 0 && max_tiles <= 0x7fffffffL && tables_elems >= IXTTS_TRUE_PEAK_TAPS &&
             n_gains >= 0 && out_elems >= 0 && partial_slots >= 0,
         "limiter: bad shape n_rows=%d x_elems=%ld n_reqs=%d max_tiles=%ld tables_elems=%ld n_gains=%d out_elems=%ld partial_slots=%ld", n_rows, x_elems,
         n_reqs, max_tiles, tables_elems, n_gains, out_elems, partial_slots);
  if (n_reqs == 0 || max_tiles == 0) return IXTTS_OK;
  hipLaunchKernelGGL(limiter_kernel, dim3((unsigned)max_tiles, (unsigned)n_reqs), dim3(LIM_THREADS), 0, (hipStream_t)stream, x_dev, x_elems,
                     (const long long*)rows_dev, n_rows, (const long long*)lreqs_dev, ceilings_dev, tables_dev, tables_elems, gains_dev, n_gains, out_dev,
                     out_elems, (unsigned int*)partials_dev, partial_slots);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}
