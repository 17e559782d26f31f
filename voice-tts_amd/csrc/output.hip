// output.hip -- the output stage after the vocoder: band-limited resampling of packed rows of unequal length, and the assembly of
// the rows of a call, with their interval silence, into one PCM buffer of the requested sample encoding; for a request that asks for
// a level, the programme loudness (ITU-R BS.1770-4) and sample peak of what it delivers, and the gain that assembly then applies.
//
// Resampler and assembly are bound by bytes and launch overhead, not arithmetic, the loudness measurement by one wave's chain of
// dependent fp64 steps: one launch serves every row (every request) of a call, the row layout comes from a device table of
// (src offset, n, dst offset) triples (int64, in elements), and nothing is allocated here.
#include "common.h"

namespace ixtts {

constexpr int RS_TILE = IXTTS_RESAMPLE_TILE;  // output samples of one workgroup
constexpr int RS_THREADS = 256;
constexpr int RS_LDS_MAX = 64 * 1024;
static_assert(RS_TILE % RS_THREADS == 0, "every thread owns RS_TILE / RS_THREADS samples of a tile");

// ---------------------------------------------------------------------------------------------------------------- resampler
// torchaudio's sinc_interp_hann resampler (prompt.sinc_resample): output j = q * new + p of a row is sum_k h[p][k] xpad[q * orig + k],
// xpad = the row behind `width` zeros, zeros after it.  The non-zero taps of a phase are contiguous in the fp32 table, so the host
// hands over compacted bands: band[p][0 .. L) = h[p][start[p] .. start[p] + L).  A workgroup stages the whole band table (row stride
// Ls, odd: adjacent phases in adjacent lanes hit different banks) and the input window of its tile in LDS, zeros where the window
// leaves the row.  A sample is ONE fma chain k = 0 .. L-1 from 0.0f over values that depend on its row alone: the same bits alone,
// in any batch, at any position.
__global__ __launch_bounds__(RS_THREADS) void resample_varlen_kernel(const float* __restrict__ x, long x_elems, float* __restrict__ y, long y_elems,
                                                                     const long long* __restrict__ rows, const float* __restrict__ bands,
                                                                     const int* __restrict__ starts, int orig, int new_, int width, int L, int Ls) {
  extern __shared__ __align__(16) float rs_lds[];
  const long long src = rows[3 * blockIdx.y], n = rows[3 * blockIdx.y + 1], dst = rows[3 * blockIdx.y + 2];
  if (n <= 0) return;
  const long long out_n = (n * new_ + orig - 1) / orig;
  const long long j0 = (long long)blockIdx.x * RS_TILE;
  if (j0 >= out_n) return;  // (the grid is cut for the longest row)
  // a row the buffers cannot hold is left alone: nothing is read or written outside [0, x_elems) / [0, y_elems)
  if (src < 0 || dst < 0 || src + n > x_elems || dst + out_n > y_elems || out_n > 0x7fffffffLL) return;
  const int tid = threadIdx.x;
  const int tile = (int)(out_n - j0 < RS_TILE ? out_n - j0 : RS_TILE);
  const int nb = new_ * Ls;           // floats of the band table
  const int nb4 = (nb + 3) & ~3;      // (the host pads the table to whole float4s)
  float* sb = rs_lds;
  float* sw = rs_lds + nb4;
  for (int i = tid; i < nb4 / 4; i += RS_THREADS) ((float4*)sb)[i] = ((const float4*)bands)[i];
  const long long q0 = j0 / new_, q1 = (j0 + tile - 1) / new_;
  const int K = 2 * width + orig;
  const int wlen = (int)(q1 - q0) * orig + K;  // xpad[q0 * orig .. q1 * orig + K)
  int* sst = (int*)(sw + wlen);                // the phases' band starts, behind the window
  const long long x0 = q0 * orig - width;      // index into the row of the window's first sample
  for (int i = tid; i < wlen; i += RS_THREADS) {
    const long long xi = x0 + i;
    sw[i] = (xi >= 0 && xi < n) ? x[src + xi] : 0.0f;
  }
  for (int i = tid; i < new_; i += RS_THREADS) sst[i] = min(max(starts[i], 0), K - L);  // a band never leaves the window
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RS_TILE / RS_THREADS; ++r) {
    const int t = tid + r * RS_THREADS;
    if (t >= tile) break;
    const long long j = j0 + t;
    const int q = (int)(j / new_ - q0), p = (int)(j % new_);
    const float* h = sb + p * Ls;
    const float* w = sw + q * orig + sst[p];
    float acc = 0.0f;
    for (int k = 0; k < L; ++k) acc = __fmaf_rn(h[k], w[k], acc);
    y[dst + j] = fminf(fmaxf(acc, -32767.0f), 32767.0f);
  }
}

// ------------------------------------------------------------------------------------------------------- assemble and convert
// ITU-T G.711 of a 16-bit sample, as audioop.lin2ulaw / lin2alaw compute it (the 14- / 13-bit value is the sample shifted right
// arithmetically).
__device__ __forceinline__ unsigned int g711_ulaw(int s) {
  int v = s >> 2;
  const unsigned int mask = v < 0 ? 0x7Fu : 0xFFu;
  if (v < 0) v = -v;
  if (v > 8159) v = 8159;
  v += 0x21;
  const int seg = max(0, 26 - __clz(v));  // first segment end (0x3F << seg) that holds v
  if (seg >= 8) return 0x7Fu ^ mask;
  return ((unsigned int)(seg << 4) | ((unsigned int)(v >> (seg + 1)) & 0xFu)) ^ mask;
}
__device__ __forceinline__ unsigned int g711_alaw(int s) {
  int v = s >> 3;
  const unsigned int mask = v >= 0 ? 0xD5u : 0x55u;
  if (v < 0) v = -v - 1;
  const int seg = max(0, 27 - __clz(v));  // first segment end (0x1F << seg) that holds v; v = 0: clz = 32
  if (seg >= 8) return 0x7Fu ^ mask;
  const unsigned int a = (unsigned int)(seg << 4) | ((unsigned int)(v >> (seg < 2 ? 1 : seg)) & 0xFu);
  return a ^ mask;
}

// the int16 `.type(torch.int16)` gives on the host: truncation toward zero, here behind a clamp to the int16 range
__device__ __forceinline__ int pcm_s16(float v) { return (int)fminf(fmaxf(v, -32768.0f), 32767.0f); }

template <int ENC>
__device__ __forceinline__ unsigned int pcm_code(float v) {
  const int s = pcm_s16(v);
  if (ENC == IXTTS_PCM_S16LE) return (unsigned int)s & 0xFFFFu;
  if (ENC == IXTTS_PCM_MULAW) return g711_ulaw(s);
  return g711_alaw(s);
}
template <int ENC>
__device__ __forceinline__ unsigned int pcm_zero() {
  return ENC == IXTTS_PCM_S16LE ? 0u : ENC == IXTTS_PCM_MULAW ? 0xFFu : 0xD5u;
}

// Output sample i of [0, total): the row whose [dst, dst + n) holds it (rows ascending in dst, disjoint), else the code for silence.
// A thread owns four consecutive samples and stores them as one word (u8) or two (s16); `out` is 8-byte aligned.
// GAIN: rows of four columns (src, n, dst, gain index) instead of three: a sample of a row whose index lies in [0, n_gains) is the
// conversion of the fp32 product gain * x, rounded once; any other index converts x as it is.
template <int ENC, bool GAIN>
__global__ __launch_bounds__(256) void pcm_assemble_kernel(const float* __restrict__ x, long x_elems, void* __restrict__ out, long total,
                                                           const long long* __restrict__ rows, int n_rows, const float* __restrict__ gains,
                                                           int n_gains) {
  constexpr int COLS = GAIN ? 4 : 3;
  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= total) return;
  // the last row with dst <= i0 (-1: none)
  int lo = -1, hi = n_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[COLS * mid + 2] <= (long long)i0) lo = mid;
    else hi = mid - 1;
  }
  int r = lo;
  long long src = 0, n = 0, dst = 0, gi = -1;
  if (r >= 0) {
    src = rows[COLS * r]; n = rows[COLS * r + 1]; dst = rows[COLS * r + 2];
    if constexpr (GAIN) gi = rows[COLS * r + 3];
  }
  bool scaled = false;
  float g = 1.0f;
  if constexpr (GAIN) {
    scaled = gi >= 0 && gi < n_gains;
    g = scaled ? gains[gi] : 1.0f;
  }
  unsigned int c[4];
  // all four in one row, 16-byte aligned in the input: one load
  const long long s0 = src + (i0 - dst);
  const bool quad = r >= 0 && i0 + 3 - dst < n && src >= 0 && s0 + 3 < x_elems && ((uintptr_t)(x + s0) & 15) == 0 && (r + 1 >= n_rows || rows[COLS * (r + 1) + 2] > i0 + 3);
  if (quad) {
    float4 v = *(const float4*)(x + s0);
    if constexpr (GAIN) {
      if (scaled) { v.x = __fmul_rn(g, v.x); v.y = __fmul_rn(g, v.y); v.z = __fmul_rn(g, v.z); v.w = __fmul_rn(g, v.w); }
    }
    c[0] = pcm_code<ENC>(v.x); c[1] = pcm_code<ENC>(v.y); c[2] = pcm_code<ENC>(v.z); c[3] = pcm_code<ENC>(v.w);
  }
#pragma unroll
  for (int e = 0; e < 4 && !quad; ++e) {
    const long long i = i0 + e;
    // step to the next row once i reaches its dst (rows of n = 0 are stepped over)
    while (r + 1 < n_rows && rows[COLS * (r + 1) + 2] <= i) {
      ++r;
      src = rows[COLS * r]; n = rows[COLS * r + 1]; dst = rows[COLS * r + 2];
      if constexpr (GAIN) {
        gi = rows[COLS * r + 3];
        scaled = gi >= 0 && gi < n_gains;
        g = scaled ? gains[gi] : 1.0f;
      }
    }
    const long long s = src + (i - dst);
    const bool in = r >= 0 && i - dst < n && src >= 0 && s < x_elems;  // (a source outside the input reads as silence)
    if constexpr (GAIN) c[e] = in ? pcm_code<ENC>(scaled ? __fmul_rn(g, x[s]) : x[s]) : pcm_zero<ENC>();
    else c[e] = in ? pcm_code<ENC>(x[s]) : pcm_zero<ENC>();
  }
  if (i0 + 4 <= total) {
    if (ENC == IXTTS_PCM_S16LE) *(uint2*)((unsigned short*)out + i0) = make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
    else *(unsigned int*)((unsigned char*)out + i0) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  } else {
    for (int e = 0; e < 4 && i0 + e < total; ++e) {
      if (ENC == IXTTS_PCM_S16LE) ((unsigned short*)out)[i0 + e] = (unsigned short)c[e];
      else ((unsigned char*)out)[i0 + e] = (unsigned char)c[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------- programme loudness (BS.1770-4)
// The K-weighted energy of every hop (100 ms) of every request, and the sample peak of the hop.  One wave per hop: it stages the
// window of the programme from R = H + H / 2 samples before its hop to the hop's end in LDS (zeros in the gaps, before the start
// and behind the end) and filters it from zero state at the window's start, in three steps over chunks of Cw = ceil((R + H) / 64) | 1
// samples, one per lane (odd: the lanes' reads fall into different LDS banks):
//   1. every lane filters its chunk from zero state and keeps the state it ends in, v_l;
//   2. the filter is linear, so the state lane l must START from is S_l = M S_(l-1) + v_(l-1), S_0 = 0, with M = A^Cw the
//      zero-input transition of the cascade's four state variables over one chunk (fp64, from the host, per request);
//   3. every lane filters its chunk again, from S_l, and sums the squares of the outputs that fall into the hop.
// That is the sequential filter over the window, 2 Cw dependent steps per lane instead of R + H.  What the window leaves out is the
// state at its start: the slowest pole is the high-pass's double pole, radius r = e^(-2 pi 38.1 / fs), and what a state of size S
// leaves after n samples is about S (1 + n (1 - r)) r^n -- 25 S 4e-11 = 1e-9 S after one hop at any rate, which a 45 Hz tone turns
// into 1.2e-9 of a hop's energy, and 36 S 2.5e-16 = 1e-14 S after a hop and a half.  Before the programme's start the window holds
// zeros from zero state, which is exact.  Recursion and sums are fp64; the 64 partial sums are added in lane order.
constexpr int LM_LANES = 64;
constexpr int LM_MAX_HOP = IXTTS_LOUDNESS_MAX_HOP;
constexpr int LM_WINDOW = LM_MAX_HOP + LM_MAX_HOP / 2 + LM_MAX_HOP;

struct KWeight {
  double b0, b1, b2, a1, a2;  // the shelf, b already times 2^-15 (exact): samples enter on the +-32767 scale
  double h1, h2;              // the high-pass: a1, a2 (b = 1, -2, 1)
  double s1 = 0.0, s2 = 0.0, u1 = 0.0, u2 = 0.0;
  // transposed direct form II, both sections
  __device__ __forceinline__ double step(double x) {
    const double y = fma(b0, x, s1);
    s1 = fma(-a1, y, fma(b1, x, s2));
    s2 = fma(-a2, y, b2 * x);
    const double z = y + u1;
    u1 = fma(-h1, z, fma(-2.0, y, u2));
    u2 = fma(-h2, z, y);
    return z;
  }
};

__global__ __launch_bounds__(LM_LANES) void loudness_measure_kernel(const float* __restrict__ x, long x_elems, const long long* __restrict__ rows, int n_rows,
                                                                    const long long* __restrict__ reqs, const double* __restrict__ coefs,
                                                                    double* __restrict__ energy, float* __restrict__ hop_peak, long hops_elems) {
  __shared__ float w[LM_WINDOW];  // programme [t0 - R, t0 + H)
  __shared__ double part[LM_LANES];
  __shared__ double ends[LM_LANES][4];
  const long long* rq = reqs + (long)blockIdx.y * IXTTS_LOUDNESS_REQ_COLS;
  const long long row_lo = rq[0], nr = rq[1], start = rq[2], extent = rq[3], H64 = rq[4], slot = rq[5] + blockIdx.x;
  if (H64 <= 0 || H64 > LM_MAX_HOP || extent <= 0) return;
  const int H = (int)H64;
  const long long t0 = (long long)blockIdx.x * H;
  if (t0 >= extent) return;  // (the grid is cut for the request with the most hops)
  if (slot < 0 || slot >= hops_elems || row_lo < 0 || nr < 0 || row_lo + nr > n_rows) return;
  const int lane = threadIdx.x;
  const int R = H + H / 2;
  for (int i = lane; i < R + H; i += LM_LANES) w[i] = 0.0f;
  __syncthreads();
  // every row of the request that reaches into the window (rows are disjoint: no sample is written twice)
  const long long w0 = start + t0 - R, w1 = min(start + t0 + H, start + extent);  // the window in the coordinate of dst
  for (long long r = row_lo; r < row_lo + nr; ++r) {
    const long long src = rows[3 * r], n = rows[3 * r + 1], dst = rows[3 * r + 2];
    const long long a = max(max(dst, w0), start), b = min(dst + n, w1);
    if (n <= 0 || a >= b || src < 0 || src + n > x_elems) continue;  // (a source outside the input reads as silence)
    const float* xs = x + src + (a - dst);
    float* ws = w + (a - w0);
    const int len = (int)(b - a);
    for (int i = lane; i < len; i += LM_LANES) ws[i] = xs[i];
  }
  __syncthreads();
  const double* cf = coefs + (long)blockIdx.y * IXTTS_LOUDNESS_COEF_COLS;
  const double scale = 1.0 / 32768.0;
  KWeight f;
  f.b0 = cf[0] * scale; f.b1 = cf[1] * scale; f.b2 = cf[2] * scale; f.a1 = cf[3]; f.a2 = cf[4]; f.h1 = cf[5]; f.h2 = cf[6];
  const int valid = (int)min((long long)H, extent - t0);  // samples the hop has (a trailing partial hop: fewer than H)
  const int Cw = ((R + H + LM_LANES - 1) / LM_LANES) | 1;
  const int c0 = min(lane * Cw, R + valid), c1 = min(c0 + Cw, R + valid);
  // 1. the chunk from zero state: its end state
#pragma unroll 4
  for (int i = c0; i < c1; ++i) f.step((double)w[i]);
  ends[lane][0] = f.s1; ends[lane][1] = f.s2; ends[lane][2] = f.u1; ends[lane][3] = f.u2;
  __syncthreads();
  // 2. the state the chunk starts from (every chunk before this lane's is a whole one: only the last may be short)
  double S[4] = {0.0, 0.0, 0.0, 0.0};
  const double* M = cf + 8;  // row-major 4 x 4
  for (int l = 0; l < lane; ++l) {
    double T[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) T[a] = fma(M[4 * a + 3], S[3], fma(M[4 * a + 2], S[2], fma(M[4 * a + 1], S[1], fma(M[4 * a], S[0], ends[l][a]))));
#pragma unroll
    for (int a = 0; a < 4; ++a) S[a] = T[a];
  }
  // 3. the chunk from that state: the energy of what falls into the hop
  f.s1 = S[0]; f.s2 = S[1]; f.u1 = S[2]; f.u2 = S[3];
  double acc = 0.0;
  const int mid = min(max(c0, R), c1);
  for (int i = c0; i < mid; ++i) f.step((double)w[i]);
#pragma unroll 4
  for (int i = mid; i < c1; ++i) {
    const double y = f.step((double)w[i]);
    acc = fma(y, y, acc);
  }
  float p = 0.0f;
  for (int i = lane; i < valid; i += LM_LANES) p = fmaxf(p, fabsf(w[R + i]));
  p = wave_max(p);
  part[lane] = acc;
  __syncthreads();
  if (lane == 0) {
    double e = 0.0;
    for (int l = 0; l < LM_LANES; ++l) e += part[l];
    energy[slot] = e;
    hop_peak[slot] = p;
  }
}

// Gating and gain of one request: the blocks of four hops, the two gates, the integrated loudness, the gain for the target and the
// ceiling.  One wave; a lane sums its blocks j = lane, lane + 64, ... in that order and the 64 partial sums are added in lane order.
__device__ __forceinline__ void gate_pass(const double* __restrict__ e, int nb, double inv, double gate, int lane, double* sum, int* cnt, double& S, int& N) {
  double s = 0.0;
  int c = 0;
  for (int j = lane; j < nb; j += LM_LANES) {
    const double z = (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) * inv;
    const double l = -0.691 + 10.0 * log10(z);
    if (l > -70.0 && l > gate) { s += z; ++c; }
  }
  __syncthreads();  // (the arrays of the pass before have been read)
  sum[lane] = s;
  cnt[lane] = c;
  __syncthreads();
  S = 0.0;
  N = 0;
  for (int l = 0; l < LM_LANES; ++l) { S += sum[l]; N += cnt[l]; }
}

__global__ __launch_bounds__(LM_LANES) void loudness_gain_kernel(const double* __restrict__ energy, const float* __restrict__ hop_peak, long hops_elems,
                                                                 const long long* __restrict__ reqs, const double* __restrict__ targets,
                                                                 ixtts_loudness_record* __restrict__ records, float* __restrict__ gains) {
  __shared__ double sum[LM_LANES];
  __shared__ int cnt[LM_LANES];
  const int q = blockIdx.x, lane = threadIdx.x;
  const long long* rq = reqs + (long)q * IXTTS_LOUDNESS_REQ_COLS;
  const long long extent = rq[3], H = rq[4], slot0 = rq[5];
  long long hops = 0, full = 0;
  if (H > 0 && H <= LM_MAX_HOP && extent > 0) { hops = (extent + H - 1) / H; full = extent / H; }
  if (slot0 < 0 || slot0 + hops > hops_elems || hops > 0x7fffffffLL) hops = full = 0;  // hops the arrays do not hold: nothing measured
  float p = 0.0f;
  for (long long k = lane; k < hops; k += LM_LANES) p = fmaxf(p, hop_peak[slot0 + k]);
  p = wave_max(p);
  const int nb = full >= 4 ? (int)(full - 3) : 0;
  const double* e = energy + slot0;
  const double inv = H > 0 ? 1.0 / (4.0 * (double)H) : 0.0;
  double S, S2;
  int N, N2 = 0;
  gate_pass(e, nb, inv, -70.0, lane, sum, cnt, S, N);
  double L = __builtin_nan("");
  if (N > 0) {
    const double gamma = -0.691 + 10.0 * log10(S / N) - 10.0;
    gate_pass(e, nb, inv, gamma, lane, sum, cnt, S2, N2);
    if (N2 > 0) L = -0.691 + 10.0 * log10(S2 / N2);
  }
  if (lane != 0) return;
  const double target = targets[2 * q], ceiling_db = targets[2 * q + 1];
  unsigned int flags = N2 > 0 ? 0u : IXTTS_LOUDNESS_NO_BLOCK;
  double g = 1.0;
  if (target == target && N2 > 0) g = pow(10.0, (target - L) / 20.0);
  if (ceiling_db == ceiling_db) {
    const double c = 32768.0 * pow(10.0, ceiling_db / 20.0);
    if (g * (double)p > c) { g = c / (double)p; flags |= IXTTS_LOUDNESS_CEILING_BOUND; }
  }
  ixtts_loudness_record rec;
  rec.lufs = L;
  rec.gain = (float)g;
  rec.peak = p;
  rec.flags = flags;
  rec.blocks = (uint32_t)nb;
  records[q] = rec;
  gains[q] = (float)g;
}

}  // namespace ixtts

using namespace ixtts;

extern "C" int ixtts_resample_tile(void) { return RS_TILE; }

extern "C" int ixtts_resample_varlen_f32(const float* x_dev, long x_elems, float* y_dev, long y_elems, const int64_t* rows_dev, int n_rows, long max_n,
                                         const float* bands_dev, long bands_elems, const int* starts_dev, int orig, int new_, int width, int band, void* stream) {
  IX_ARG(x_dev && y_dev && rows_dev && bands_dev && starts_dev, "resample_varlen: null pointer");
  IX_ARG(n_rows >= 0 && n_rows <= 65535 && max_n >= 0 && x_elems >= 0 && y_elems >= 0, "resample_varlen: bad shape n_rows=%d max_n=%ld x_elems=%ld y_elems=%ld",
         n_rows, max_n, x_elems, y_elems);
  IX_ARG(orig > 0 && new_ > 0 && width > 0 && band > 0 && band <= 2 * width + orig, "resample_varlen: bad table orig=%d new=%d width=%d band=%d", orig,
         new_, width, band);
  IX_ARG(((uintptr_t)bands_dev & 15) == 0, "resample_varlen: the band table must be 16-byte aligned");
  if (n_rows == 0 || max_n == 0) return IXTTS_OK;
  const long max_out = (long)(((__int128)max_n * new_ + orig - 1) / orig);
  IX_ARG(max_out <= 0x7fffffffL, "resample_varlen: a row of %ld samples gives more than 2^31 - 1 output samples", max_n);
  const int Ls = band | 1;
  const long nb4 = ((long)new_ * Ls + 3) & ~3L;
  IX_ARG(bands_elems >= nb4, "resample_varlen: the band table holds %ld floats, %d phases of %d taps (row stride %d, padded to 4) need %ld", bands_elems,
         new_, band, Ls, nb4);
  const long wmax = ((long)(RS_TILE - 1) / new_ + 1) * orig + 2L * width + orig;  // the longest window of a tile
  const long lds = (nb4 + wmax + new_) * 4;
  IX_ARG(lds <= RS_LDS_MAX, "resample_varlen: %d/%d needs %ld bytes of LDS (limit %d)", orig, new_, lds, RS_LDS_MAX);
  const dim3 grid((unsigned)((max_out + RS_TILE - 1) / RS_TILE), (unsigned)n_rows);
  hipLaunchKernelGGL(resample_varlen_kernel, grid, dim3(RS_THREADS), (size_t)lds, (hipStream_t)stream, x_dev, x_elems, y_dev, y_elems,
                     (const long long*)rows_dev, bands_dev, starts_dev, orig, new_, width, band, Ls);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

// the checks and the launch of both assemble entries; `who` names the entry in the messages
template <bool GAIN>
static int pcm_assemble_host(const char* who, const float* x_dev, long x_elems, void* out_dev, long total, const int64_t* rows_dev, int n_rows,
                             const float* gains_dev, int n_gains, int encoding, void* stream) {
  IX_ARG(out_dev && rows_dev && (x_dev || x_elems == 0) && (gains_dev || n_gains == 0), "%s: null pointer", who);
  if constexpr (GAIN) {
    IX_ARG(n_rows >= 0 && total >= 0 && x_elems >= 0 && n_gains >= 0, "%s: bad shape n_rows=%d total=%ld x_elems=%ld n_gains=%d", who, n_rows, total,
           x_elems, n_gains);
  } else {
    IX_ARG(n_rows >= 0 && total >= 0 && x_elems >= 0, "%s: bad shape n_rows=%d total=%ld x_elems=%ld", who, n_rows, total, x_elems);
  }
  IX_ARG(encoding == IXTTS_PCM_S16LE || encoding == IXTTS_PCM_MULAW || encoding == IXTTS_PCM_ALAW, "%s: unknown encoding %d", who, encoding);
  IX_ARG(((uintptr_t)out_dev & 7) == 0, "%s: the output buffer must be 8-byte aligned", who);
  if (total == 0) return IXTTS_OK;
  auto* kernel = encoding == IXTTS_PCM_S16LE ? pcm_assemble_kernel<IXTTS_PCM_S16LE, GAIN>
               : encoding == IXTTS_PCM_MULAW ? pcm_assemble_kernel<IXTTS_PCM_MULAW, GAIN>
                                             : pcm_assemble_kernel<IXTTS_PCM_ALAW, GAIN>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, x_dev, x_elems, out_dev, total,
                     (const long long*)rows_dev, n_rows, gains_dev, n_gains);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

extern "C" int ixtts_pcm_assemble(const float* x_dev, long x_elems, void* out_dev, long total, const int64_t* rows_dev, int n_rows, int encoding,
                                  void* stream) {
  return pcm_assemble_host<false>("pcm_assemble", x_dev, x_elems, out_dev, total, rows_dev, n_rows, nullptr, 0, encoding, stream);
}

extern "C" int ixtts_pcm_assemble_gain(const float* x_dev, long x_elems, void* out_dev, long total, const int64_t* rows_dev, int n_rows,
                                       const float* gains_dev, int n_gains, int encoding, void* stream) {
  return pcm_assemble_host<true>("pcm_assemble_gain", x_dev, x_elems, out_dev, total, rows_dev, n_rows, gains_dev, n_gains, encoding, stream);
}

extern "C" int ixtts_loudness_measure(const float* x_dev, long x_elems, const int64_t* rows_dev, int n_rows, const int64_t* reqs_dev, const double* coefs_dev,
                                      int n_reqs, long max_hops, double* energy_dev, float* hop_peak_dev, long hops_elems, void* stream) {
  IX_ARG(rows_dev && reqs_dev && coefs_dev && energy_dev && hop_peak_dev && (x_dev || x_elems == 0), "loudness_measure: null pointer");
  IX_ARG(n_rows >= 0 && x_elems >= 0 && n_reqs >= 0 && n_reqs <= 65535 && max_hops >= 0 && max_hops <= 0x7fffffffL && hops_elems >= 0,
         "loudness_measure: bad shape n_rows=%d x_elems=%ld n_reqs=%d max_hops=%ld hops_elems=%ld", n_rows, x_elems, n_reqs, max_hops, hops_elems);
  if (n_reqs == 0 || max_hops == 0) return IXTTS_OK;
  hipLaunchKernelGGL(loudness_measure_kernel, dim3((unsigned)max_hops, (unsigned)n_reqs), dim3(LM_LANES), 0, (hipStream_t)stream, x_dev, x_elems,
                     (const long long*)rows_dev, n_rows, (const long long*)reqs_dev, coefs_dev, energy_dev, hop_peak_dev, hops_elems);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}

extern "C" int ixtts_loudness_gain(const double* energy_dev, const float* hop_peak_dev, long hops_elems, const int64_t* reqs_dev, const double* targets_dev,
                                   int n_reqs, ixtts_loudness_record* records_dev, float* gains_dev, void* stream) {
  IX_ARG(energy_dev && hop_peak_dev && reqs_dev && targets_dev && records_dev && gains_dev, "loudness_gain: null pointer");
  IX_ARG(n_reqs >= 0 && hops_elems >= 0, "loudness_gain: bad shape n_reqs=%d hops_elems=%ld", n_reqs, hops_elems);
  IX_ARG(((uintptr_t)records_dev & 7) == 0, "loudness_gain: the records must be 8-byte aligned");
  if (n_reqs == 0) return IXTTS_OK;
  hipLaunchKernelGGL(loudness_gain_kernel, dim3((unsigned)n_reqs), dim3(LM_LANES), 0, (hipStream_t)stream, energy_dev, hop_peak_dev, hops_elems,
                     (const long long*)reqs_dev, targets_dev, records_dev, gains_dev);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}
