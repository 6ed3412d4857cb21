// mobi_rgb.h -- the per-pixel arithmetic of the Bitmap (MD.cs:260-323), shared by the kernels that compile it: mobi_yuv_to_argb
// (mobi_rgb.hip, the Bitmap itself) and the RGB tensor exports mobi_export_rgb, mobi_export_scale and mobi_export_resample (the .hip
// files of those names; the latter two through mobi_export_tensor.h).  All therefore compute the same 0xAARRGGBB word for every pixel;
// the tensor exports take their R, G, B from bytes 2, 1, 0 of that word.
//
// Per pixel: Y, plus U and V averaged from up to four chroma neighbours chosen by the pixel's parity (not on the last column / last row,
// MD.cs:269), then either the float BT.601-like matrix with the 16..255 range stretch (Moflex3DS, :297-305) or the integer Y+U-V / Y+V /
// Y-U-V form on truncated values (ModsDS, :306-311), clamp, truncate, pack as 0xAARRGGBB (:313-319).
//
// Float semantics are the reference's: IEEE single, one rounding per C# operator in source order.  Hence contraction is switched
// off where the arithmetic is (hipcc contracts a*b+c into an FMA by default, which rounds once instead of twice).
#ifndef MOBI_RGB_H
#define MOBI_RGB_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mobi_rgb {
typedef float f32x2 __attribute__((ext_vector_type(2)));
// x / 239f, correctly rounded, in three instructions instead of the ~10 of a generic IEEE division: q0 = x*r,
// q = fma(fma(-239, q0, x), r, q0) with r = RN(1/239).  Not a theorem for every divisor: it is CHECKED for this one,
// exhaustively over all 2^32 bit patterns (mobi_selftest_div239, tests/test_rgb.py): identical to __fdiv_rn for every
// float with 1e-30 <= |x| <= 1e30, and for x = 0 up to the sign of zero, which the clamp and the int cast discard.
// (The stretch's numerator is (c - 16) * 255 with |c| < 1000: zero, or at least 1e-4 in magnitude.)
__device__ __forceinline__ float div239(float x) {
  const float r = 1.0f / 239.0f;
  const float q0 = __fmul_rn(x, r);
  return __fmaf_rn(__fmaf_rn(-239.0f, q0, x), r, q0);
}
// The same on two pixels at once: gfx950's packed single-precision instructions (v_pk_mul_f32, v_pk_add_f32, v_pk_fma_f32) round each
// half exactly as the scalar ones do, at twice the rate.  Contraction is OFF in these functions: a product and a sum are two roundings
// (the reference's), and only what is written as an fma is one.  (The pragma holds to the end of every file that includes this one: the
// kernels behind it compile without contraction too.)
#pragma clang fp contract(off)
__device__ __forceinline__ f32x2 div239_2(f32x2 x) {
  const f32x2 r = {1.0f / 239.0f, 1.0f / 239.0f}, m = {-239.0f, -239.0f};
  const f32x2 q0 = x * r;
  return __builtin_elementwise_fma(__builtin_elementwise_fma(m, q0, x), r, q0);
}
__device__ __forceinline__ f32x2 stretch2(f32x2 c) { // (c - 16f) * 255f / (255f - 16f), MD.cs:303-305
  const f32x2 k16 = {16.f, 16.f}, k255 = {255.f, 255.f};
  return div239_2((c - k16) * k255);
}
// clamp to [0, 255], truncate, place in byte `pos` of `old` (MD.cs:313-319).  v_cvt_pk_u8_f32 saturates to [0, 255] but rounds to
// nearest; behind a floor it has nothing left to round, and below zero floor and truncation differ only where both saturate to 0:
// identical to the comparison chain for every float that is not a NaN (tools/ubench/cvtpk.hip, all 2^32 patterns; alone it differs
// for 41.9 M of them, 0.5000001 first).  Two instructions per output byte instead of five.
template <int POS>
__device__ __forceinline__ uint32_t put_u8(float x, uint32_t old) {
  uint32_t d = old;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_cvt_pk_u8_f32 %0, %1, %2, %0" : "+v"(d) : "v"(__builtin_floorf(x)), "n"(POS));
#endif
  return d;
}
__device__ __forceinline__ int clamp255(int x) { return x < 0 ? 0 : x > 255 ? 255 : x; }
// two pixels: luma bytes y0, y1 (as floats), chroma numerators in quarter samples (see chroma_numerators)
__device__ __forceinline__ void convert2(int version, f32x2 Y2, int un0, int un1, int vn0, int vn1, uint32_t &p0, uint32_t &p1) {
  if (version == 2) { // Moflex3DS: the float matrix and the 16..255 stretch (MD.cs:297-305)
    const f32x2 q = {0.25f, 0.25f};
    const f32x2 U = f32x2{(float)un0, (float)un1} * q, V = f32x2{(float)vn0, (float)vn1} * q; // exact: small integers, a power of two
    const f32x2 kRV = {1.420f, 1.420f}, kGU = {0.344f, 0.344f}, kGV = {0.714f, 0.714f}, kBU = {1.772f, 1.772f};
    const f32x2 R = stretch2(Y2 + kRV * V);
    const f32x2 G = stretch2((Y2 - kGU * U) - kGV * V);
    const f32x2 B = stretch2(Y2 + kBU * U);
    p0 = put_u8<2>(R.x, put_u8<1>(G.x, put_u8<0>(B.x, 0xFF000000u))); // Color.FromArgb(r, g, b).ToArgb()
    p1 = put_u8<2>(R.y, put_u8<1>(G.y, put_u8<0>(B.y, 0xFF000000u)));
    return;
  }
  // ModsDS: (int) casts truncate toward zero; y + u - v, y + v, y - u - v on the truncated values (MD.cs:306-311)
  auto tz = [](int n) { return n >= 0 ? n >> 2 : -((-n) >> 2); };
  const int u0 = tz(un0), u1 = tz(un1), v0 = tz(vn0), v1 = tz(vn1), y0 = (int)Y2.x, y1 = (int)Y2.y;
  p0 = 0xFF000000u | ((uint32_t)clamp255(y0 + u0 - v0) << 16) | ((uint32_t)clamp255(y0 + v0) << 8) | (uint32_t)clamp255(y0 - u0 - v0);
  p1 = 0xFF000000u | ((uint32_t)clamp255(y1 + u1 - v1) << 16) | ((uint32_t)clamp255(y1 + v1) << 8) | (uint32_t)clamp255(y1 - u1 - v1);
}
// Chroma (MD.cs:262-296) of four pixels x0 .. x0 + 3 (x0 a multiple of 4) in an even row y0 and the odd row y0 + 1 below it: a pixel takes
// the sample under it, or -- not in the picture's last column or last row -- the mean of that sample and its right / lower / three
// neighbours, by the pixel's parity.  The samples are bytes minus 128 and the means divide by 2 or 4, so every intermediate float of the
// reference is an exact small multiple of 1/4: the numerators are added as integers (4a, 2(a + b), a + b + c + d, minus 512) and one
// exact multiplication by 0.25 (convert2) gives the float the reference's additions and division give.
//   w0 = the samples a, b under the four pixels in the chroma row y0 / 2 (byte 0, byte 1), e0w = the sample e right of b (byte 0);
//   w1, e1w = the same in the chroma row below (not looked at when lastrow).
//   lastrow: y0 + 1 is the picture's last row; lastcol: x0 + 3 is its last column (e0w, e1w not looked at).
// ev = numerators of the even row's pixels, od = of the odd row's: 4a, 2(a + b), 4b, 2(b + e) and 2(a + a'), a + b + a' + b', 2(b + b'),
// b + e + b' + e' (all minus 4 * 128).
__device__ __forceinline__ void chroma_numerators(uint32_t w0, uint32_t e0w, uint32_t w1, uint32_t e1w, bool lastrow, bool lastcol, int (&ev)[4],
                                                  int (&od)[4]) {
  const int a0 = (int)(w0 & 0xFF), b0 = (int)(w0 >> 8) & 0xFF, e0 = (int)(e0w & 0xFF), a1 = (int)(w1 & 0xFF), b1 = (int)(w1 >> 8) & 0xFF, e1 = (int)(e1w & 0xFF);
  const int pa = 4 * a0 - 512, pb = 4 * b0 - 512; // the plain sample
  ev[0] = pa; ev[1] = 2 * (a0 + b0) - 512; ev[2] = pb; ev[3] = lastcol ? pb : 2 * (b0 + e0) - 512;
  od[0] = 2 * (a0 + a1) - 512; od[1] = a0 + b0 + a1 + b1 - 512; od[2] = 2 * (b0 + b1) - 512; od[3] = lastcol ? pb : b0 + e0 + b1 + e1 - 512;
  if (lastrow) { od[0] = pa; od[1] = pa; od[2] = pb; od[3] = pb; } // the odd row is the picture's last: no mean of any kind (MD.cs:269)
}
// The Bitmap's words of those four pixels in both rows, pe = the even row's, po = the odd row's: yw0, yw1 = their luma bytes, the chroma
// words and lastrow / lastcol as in chroma_numerators (u.. of the U plane, v.. of the V plane).  The lane shape of mobi_yuv_to_argb and
// of fetch_quad (mobi_export_tensor.h); how the words are fetched is the caller's.
__device__ __forceinline__ void convert_quad(int version, uint32_t yw0, uint32_t yw1, uint32_t u0w, uint32_t ue0, uint32_t u1w, uint32_t ue1, uint32_t v0w,
                                             uint32_t ve0, uint32_t v1w, uint32_t ve1, bool lastrow, bool lastcol, uint32_t (&pe)[4], uint32_t (&po)[4]) {
  int ue[4], uo[4], ve[4], vo[4];
  chroma_numerators(u0w, ue0, u1w, ue1, lastrow, lastcol, ue, uo);
  chroma_numerators(v0w, ve0, v1w, ve1, lastrow, lastcol, ve, vo);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const f32x2 ye = {(float)((yw0 >> (16 * k)) & 0xFF), (float)((yw0 >> (16 * k + 8)) & 0xFF)};
    const f32x2 yo = {(float)((yw1 >> (16 * k)) & 0xFF), (float)((yw1 >> (16 * k + 8)) & 0xFF)};
    convert2(version, ye, ue[2 * k], ue[2 * k + 1], ve[2 * k], ve[2 * k + 1], pe[2 * k], pe[2 * k + 1]);
    convert2(version, yo, uo[2 * k], uo[2 * k + 1], vo[2 * k], vo[2 * k + 1], po[2 * k], po[2 * k + 1]);
  }
}
// One element of an RGB tensor (the three export kernels) from the byte value v of channel ch (0 R, 1 G, 2 B), as the
// bits of ESIZE bytes: uint8 is v; float32 is (float)v * sb[ch] + sb[3 + ch]; float16 is that float32 value rounded to nearest-even
// (v_cvt_f16_f32 in the default rounding mode).
// a product and a sum, each rounded: written here, under contract(off) -- __fmul_rn / __fadd_rn are plain operators in the HIP headers,
// compiled where contraction is on, and the backend fused them into one v_fma_f32
template <int ESIZE>
__device__ __forceinline__ uint32_t tensor_element(uint32_t v, int ch, const float (&sb)[6]) {
  if (ESIZE == 1) return v;
  float f;
  {
#pragma clang fp contract(off)
    const float p = (float)v * sb[ch];
    f = p + sb[3 + ch];
  }
  return ESIZE == 2 ? (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f) : __float_as_uint(f);
}
} // namespace mobi_rgb

#endif
