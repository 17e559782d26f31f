// common.h -- shared host/device helpers for libixtts_hip.so (gfx950 only).
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>

#include "../../include/ixtts_hip.h"

namespace ixtts {

// ---- error plumbing: no exceptions across the ABI ---------------------------------
void set_error(const char* fmt, ...);

#define IX_HIP(expr)                                                                   \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) {                                                            \
      ::ixtts::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return IXTTS_ERR_HIP;                                                            \
    }                                                                                  \
  } while (0)

#define IX_ARG(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      ::ixtts::set_error(__VA_ARGS__);     \
      return IXTTS_ERR_ARG;                \
    }                                      \
  } while (0)

#define IX_TRY(expr)            \
  do {                          \
    int _r = (expr);            \
    if (_r != IXTTS_OK) return _r; \
  } while (0)

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- device helpers -------------------------------------------------------------
typedef __hip_bfloat16 bf16;

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
  return __uint_as_float(((unsigned int)b) << 16);
}
// Packed (ragged) sequences: off[0 .. n] ascending, sequence s owns rows [off[s], off[s+1]).  Returns the s with
// off[s] <= row < off[s+1], clamped to [0, n-1] (rows past off[n] belong to the last sequence).
__device__ __forceinline__ int seq_of_row(const int* __restrict__ off, int n, long row) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long)off[mid] <= row) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// RoPE of one pair: (x + i y) (cos + i sin), f = (cos, sin).  The roundings are those `rope_qk_kernel` (dit_ops.hip) has always been
// compiled to -- the sine product rounded on its own, the cosine product fused with the sum -- written out so that every kernel that
// rotates (rope_qk_kernel, and the K split and Q load of attn_full_x3.hip) gives the same bits whatever the compiler contracts.
__device__ __forceinline__ float2 rope_rotate(float x, float y, float2 f) {
  return make_float2(__fmaf_rn(x, f.x, -__fmul_rn(y, f.y)), __fmaf_rn(y, f.x, __fmul_rn(x, f.y)));
}

__device__ __forceinline__ float lo_bf16(unsigned int w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_bf16(unsigned int w) { return __uint_as_float(w & 0xffff0000u); }

// ---- IEEE half (the GPT's third weight / K-V type).  Widening is exact (v_cvt_f32_f16; the high half of a dword is taken
// with an SDWA word select, so a 16-byte load unpacks in 8 instructions, as the 4 shifts + 4 ands of bf16 do).
typedef _Float16 f16;
constexpr float F16_MAX = 65504.0f;
__device__ __forceinline__ float lo_f16(unsigned int w) { return (float)__builtin_bit_cast(f16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float hi_f16(unsigned int w) { return (float)__builtin_bit_cast(f16, (unsigned short)(w >> 16)); }
// fp32 -> fp16 of an ACTIVATION, round to nearest even, saturating: a finite value never becomes inf (|v| > 65504 stores
// +-65504), and NaN cannot arise from a finite input
__device__ __forceinline__ f16 f16_sat(float v) { return (f16)__builtin_fminf(__builtin_fmaxf(v, -F16_MAX), F16_MAX); }
// 16 bytes -> 8 floats, element 2w in the low half of word w
template <typename T>
__device__ __forceinline__ void unpack8(const uint4& r, float (&o)[8]);
template <>
__device__ __forceinline__ void unpack8<bf16>(const uint4& r, float (&o)[8]) {
  o[0] = lo_bf16(r.x); o[1] = hi_bf16(r.x); o[2] = lo_bf16(r.y); o[3] = hi_bf16(r.y);
  o[4] = lo_bf16(r.z); o[5] = hi_bf16(r.z); o[6] = lo_bf16(r.w); o[7] = hi_bf16(r.w);
}
template <>
__device__ __forceinline__ void unpack8<f16>(const uint4& r, float (&o)[8]) {
  o[0] = lo_f16(r.x); o[1] = hi_f16(r.x); o[2] = lo_f16(r.y); o[3] = hi_f16(r.y);
  o[4] = lo_f16(r.z); o[5] = hi_f16(r.z); o[6] = lo_f16(r.w); o[7] = hi_f16(r.w);
}

// ---- wavefront reductions on DPP (no LDS crossbar): fixed order -> bit-reproducible.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ float dpp_take(float v) {
  // lanes disabled by the masks / reading out of range receive 0
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, BANK_MASK, true));
}
// total lands in lane 63
__device__ __forceinline__ float wave_sum63(float v) {
  float s = v + dpp_take<0x111, 0xf, 0xf>(v);  // row_shr:1
  s += dpp_take<0x112, 0xf, 0xf>(v);           // row_shr:2
  s += dpp_take<0x113, 0xf, 0xf>(v);           // row_shr:3
  s += dpp_take<0x114, 0xf, 0xe>(s);           // row_shr:4
  s += dpp_take<0x118, 0xf, 0xc>(s);           // row_shr:8
  s += dpp_take<0x142, 0xa, 0xf>(s);           // row_bcast:15
  s += dpp_take<0x143, 0xc, 0xf>(s);           // row_bcast:31
  return s;
}
// every lane ends with the total
__device__ __forceinline__ float wave_sum(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_sum63(v)), 63));
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// the same on DPP (lanes without a source keep their own value): the maximum lands in lane 63, then goes to every lane
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ float dpp_take_or_self(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, ROW_MASK, BANK_MASK, false));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  float s = fmaxf(v, dpp_take_or_self<0x111, 0xf, 0xf>(v));  // row_shr:1
  s = fmaxf(s, dpp_take_or_self<0x112, 0xf, 0xf>(v));        // row_shr:2
  s = fmaxf(s, dpp_take_or_self<0x113, 0xf, 0xf>(v));        // row_shr:3
  s = fmaxf(s, dpp_take_or_self<0x114, 0xf, 0xe>(s));        // row_shr:4
  s = fmaxf(s, dpp_take_or_self<0x118, 0xf, 0xc>(s));        // row_shr:8
  s = fmaxf(s, dpp_take_or_self<0x142, 0xa, 0xf>(s));        // row_bcast:15
  s = fmaxf(s, dpp_take_or_self<0x143, 0xc, 0xf>(s));        // row_bcast:31
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), 63));
}
// inclusive prefix sums over the wave's lanes (the scan wave_sum63 is built on), unsigned
__device__ __forceinline__ unsigned int wave_scan_u32(unsigned int v) {
  auto take = [](unsigned int x, auto ctrl, auto rm, auto bm) {
    return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, decltype(ctrl)::value, decltype(rm)::value, decltype(bm)::value, true);
  };
  using std::integral_constant;
  unsigned int s = v + take(v, integral_constant<int, 0x111>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xf>{});
  s += take(v, integral_constant<int, 0x112>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xf>{});
  s += take(v, integral_constant<int, 0x113>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xf>{});
  s += take(s, integral_constant<int, 0x114>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xe>{});
  s += take(s, integral_constant<int, 0x118>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xc>{});
  s += take(s, integral_constant<int, 0x142>{}, integral_constant<int, 0xa>{}, integral_constant<int, 0xf>{});
  s += take(s, integral_constant<int, 0x143>{}, integral_constant<int, 0xc>{}, integral_constant<int, 0xf>{});
  return s;
}

// minimum of an int over the wave (DPP), to every lane
__device__ __forceinline__ int wave_min_i32_dpp(int v) {
  auto take = [](int x, auto ctrl, auto rm, auto bm) {
    return __builtin_amdgcn_update_dpp(x, x, decltype(ctrl)::value, decltype(rm)::value, decltype(bm)::value, false);
  };
  using std::integral_constant;
  int s = min(v, take(v, integral_constant<int, 0x111>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xf>{}));
  s = min(s, take(v, integral_constant<int, 0x112>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xf>{}));
  s = min(s, take(v, integral_constant<int, 0x113>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xf>{}));
  s = min(s, take(s, integral_constant<int, 0x114>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xe>{}));
  s = min(s, take(s, integral_constant<int, 0x118>{}, integral_constant<int, 0xf>{}, integral_constant<int, 0xc>{}));
  s = min(s, take(s, integral_constant<int, 0x142>{}, integral_constant<int, 0xa>{}, integral_constant<int, 0xf>{}));
  s = min(s, take(s, integral_constant<int, 0x143>{}, integral_constant<int, 0xc>{}, integral_constant<int, 0xf>{}));
  return __builtin_amdgcn_readlane(s, 63);
}

// ---- fp32 -> three bf16 pieces (the split-product kernels: conv1d_x3.hip, attn_full_x3.hip, aa_snake.hip)
// v = h + m + l EXACTLY: each piece is the remainder before it rounded to 8 significant bits (to nearest, ties away: truncated
// pieces would all err the same way in the products that are dropped); at most 8 significant bits are left for l.  Eight values
// become three 16-byte units of eight bf16: word w of a unit = values (2w, 2w+1), value 2w in the low 16 bits.
__device__ __forceinline__ void split8_bf16x3(const float (&v)[8], uint4& ph, uint4& pm, uint4& pl) {
  unsigned int h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = __float_as_uint(v[e]) + 0x8000u;
    const float r = v[e] - __uint_as_float(h[e] & 0xffff0000u);
    m[e] = __float_as_uint(r) + 0x8000u;
    l[e] = __float_as_uint(r - __uint_as_float(m[e] & 0xffff0000u));
  }
  auto pk = [](unsigned int hi, unsigned int lo) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); };  // the high halves of both
  ph = make_uint4(pk(h[1], h[0]), pk(h[3], h[2]), pk(h[5], h[4]), pk(h[7], h[6]));
  pm = make_uint4(pk(m[1], m[0]), pk(m[3], m[2]), pk(m[5], m[4]), pk(m[7], m[6]));
  pl = make_uint4(pk(l[1], l[0]), pk(l[3], l[2]), pk(l[5], l[4]), pk(l[7], l[6]));
}


// One entry of a sequence's bias table (sequence_bias / bad_words_ids): `len` ids and the bias their completion earns.
struct SeqBiasEntry {
  int32_t len;
  int32_t ids[IXTTS_SEQ_BIAS_LEN];
  float bias;
};

}  // namespace ixtts
