// output.hip -- the output stage after the vocoder: band-limited resampling of packed rows of unequal length, and the assembly of
// the rows of a call, with their interval silence, into one PCM buffer of the requested sample encoding.
//
// Both kernels are bound by bytes and launch overhead, not arithmetic: one launch serves every row of a call, the row layout comes
// from a device table of (src offset, n, dst offset) triples (int64, in elements), and nothing is allocated here.
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
template <int ENC>
__global__ __launch_bounds__(256) void pcm_assemble_kernel(const float* __restrict__ x, long x_elems, void* __restrict__ out, long total,
                                                           const long long* __restrict__ rows, int n_rows) {
  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= total) return;
  // the last row with dst <= i0 (-1: none)
  int lo = -1, hi = n_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[3 * mid + 2] <= (long long)i0) lo = mid;
    else hi = mid - 1;
  }
  int r = lo;
  long long src = 0, n = 0, dst = 0;
  if (r >= 0) { src = rows[3 * r]; n = rows[3 * r + 1]; dst = rows[3 * r + 2]; }
  unsigned int c[4];
  // all four in one row, 16-byte aligned in the input: one load
  const long long s0 = src + (i0 - dst);
  const bool quad = r >= 0 && i0 + 3 - dst < n && src >= 0 && s0 + 3 < x_elems && ((uintptr_t)(x + s0) & 15) == 0 && (r + 1 >= n_rows || rows[3 * (r + 1) + 2] > i0 + 3);
  if (quad) {
    const float4 v = *(const float4*)(x + s0);
    c[0] = pcm_code<ENC>(v.x); c[1] = pcm_code<ENC>(v.y); c[2] = pcm_code<ENC>(v.z); c[3] = pcm_code<ENC>(v.w);
  }
#pragma unroll
  for (int e = 0; e < 4 && !quad; ++e) {
    const long long i = i0 + e;
    // step to the next row once i reaches its dst (rows of n = 0 are stepped over)
    while (r + 1 < n_rows && rows[3 * (r + 1) + 2] <= i) {
      ++r;
      src = rows[3 * r]; n = rows[3 * r + 1]; dst = rows[3 * r + 2];
    }
    const long long s = src + (i - dst);
    const bool in = r >= 0 && i - dst < n && src >= 0 && s < x_elems;  // (a source outside the input reads as silence)
    c[e] = in ? pcm_code<ENC>(x[s]) : pcm_zero<ENC>();
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

extern "C" int ixtts_pcm_assemble(const float* x_dev, long x_elems, void* out_dev, long total, const int64_t* rows_dev, int n_rows, int encoding,
                                  void* stream) {
  IX_ARG(out_dev && rows_dev && (x_dev || x_elems == 0), "pcm_assemble: null pointer");
  IX_ARG(n_rows >= 0 && total >= 0 && x_elems >= 0, "pcm_assemble: bad shape n_rows=%d total=%ld x_elems=%ld", n_rows, total, x_elems);
  IX_ARG(encoding == IXTTS_PCM_S16LE || encoding == IXTTS_PCM_MULAW || encoding == IXTTS_PCM_ALAW, "pcm_assemble: unknown encoding %d", encoding);
  IX_ARG(((uintptr_t)out_dev & 7) == 0, "pcm_assemble: the output buffer must be 8-byte aligned");
  if (total == 0) return IXTTS_OK;
  const dim3 grid((unsigned)((total + 1023) / 1024));
  const hipStream_t s = (hipStream_t)stream;
  const long long* rows = (const long long*)rows_dev;
  if (encoding == IXTTS_PCM_S16LE) hipLaunchKernelGGL(pcm_assemble_kernel<IXTTS_PCM_S16LE>, grid, dim3(256), 0, s, x_dev, x_elems, out_dev, total, rows, n_rows);
  else if (encoding == IXTTS_PCM_MULAW) hipLaunchKernelGGL(pcm_assemble_kernel<IXTTS_PCM_MULAW>, grid, dim3(256), 0, s, x_dev, x_elems, out_dev, total, rows, n_rows);
  else hipLaunchKernelGGL(pcm_assemble_kernel<IXTTS_PCM_ALAW>, grid, dim3(256), 0, s, x_dev, x_elems, out_dev, total, rows, n_rows);
  IX_HIP(hipGetLastError());
  return IXTTS_OK;
}
