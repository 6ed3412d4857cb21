// mobi_rgb.hip -- the Bitmap that MobiclipDecoder.DecodeFrame() returns (MD.cs:260-323), on the GPU.
//
// Per pixel: the arithmetic of mobi_rgb.h (shared with the tensor exports, mobi_export_*.hip).  HBM-bound: 1.5 bytes read, 4 written per
// pixel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobi_kernels.h"
#include "mobi_rgb.h"
#include "mobi_tile.h"

namespace {
using namespace mobi_rgb;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t lane_right(uint32_t v) { // the value of the lane to the right (lane + 1) inside a row of 16 lanes
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xF, 0xF, false); // row_shl:1
#else
  return v;
#endif
}
} // namespace

// One wave = two horizontally adjacent macroblocks (32 x 16 pixels); one lane = 4 pixels of two rows: lane & 7 picks the column group,
// lane >> 3 the row pair.  The planes are macroblock tiles (mobi_tile.h): a lane's two luma rows are 4 + 4 bytes of one 16-byte chunk, its
// chroma samples two bytes of one or two tile rows; a row of the wave's output is 128 contiguous bytes.
//
// Chroma and conversion: mobi_rgb.h (convert_quad) on the lane's samples of its two rows.
// r04: 29 vector instructions per pixel instead of 65 (two pixels per floating-point instruction, one conversion instruction per output
// byte instead of five, half the chroma loads per pixel) -- tools/exp_rgb.py.
extern "C" __global__ __launch_bounds__(64) void mobi_yuv_to_argb(const uint8_t *planes, uint64_t clip_bytes, uint32_t slot_bytes, int ring_base,
                                                                 int width, int height, int stride, int version, int clip0, uint32_t *out) {
  const int mbw = width >> 4, pairs = (mbw + 1) >> 1;
  const int mby = blockIdx.x / pairs, pr = blockIdx.x - mby * pairs, clip = blockIdx.z;
  const int lane = threadIdx.x, cg = lane & 7, rp = lane >> 3;
  const int mbx = 2 * pr + (cg >> 2), x0 = mbx * 16 + (cg & 3) * 4, y0 = mby * 16 + 2 * rp;
  const bool active = mbx < mbw; // (an odd number of macroblocks per row: the last wave of a row has one)
  const uint8_t *Y = planes + (size_t)(clip0 + clip) * clip_bytes + (size_t)ring_base * slot_bytes;
  const uint8_t *UV = Y + (size_t)stride * height;
  const int lgS = 31 - __builtin_clz((unsigned)stride);
  const uint32_t mbxa = active ? (uint32_t)mbx : 0u;
  // luma: rows y0, y0 + 1 are the two rows of one chunk
  const uint8_t *yp = Y + mobi_tile_y(mbxa, (uint32_t)mby, lgS) + (((rp >> 2) * 2 + ((cg & 3) >> 1)) << 6) + (((2 * rp) & 7) << 3) + ((cg & 1) << 2);
  const uint32_t yw0 = *(const uint32_t *)yp, yw1 = *(const uint32_t *)(yp + 8);
  // chroma rows y0 / 2 and, unless the lane's odd row is the picture's last, the one below (for rp == 7: in the tile below)
  const bool lastrow = y0 + 2 >= height;
  const bool lastcol = x0 + 4 >= width;
  const uint8_t *c0p = UV + mobi_tile_c(mbxa, (uint32_t)mby, lgS) + (rp << 4) + ((cg & 3) << 1);
  const uint8_t *c1p = lastrow ? c0p : rp < 7 ? c0p + 16 : UV + mobi_tile_c(mbxa, (uint32_t)mby + 1u, lgS) + ((cg & 3) << 1);
  const uint32_t u0w = *(const uint16_t *)c0p, v0w = *(const uint16_t *)(c0p + 8), u1w = *(const uint16_t *)c1p, v1w = *(const uint16_t *)(c1p + 8);
  // the sample to the right of the lane's two: the next lane's first one -- except for the wave's last column group, whose right
  // neighbour is the next pair's first macroblock (not looked at in the picture's last column)
  uint32_t ue0 = lane_right(u0w), ve0 = lane_right(v0w), ue1 = lane_right(u1w), ve1 = lane_right(v1w);
  if (cg == 7 && !lastcol) {
    const int d0 = (int)(mobi_tile_c((uint32_t)mbx + 1u, 0, lgS)) - (int)(mobi_tile_c((uint32_t)mbx, 0, lgS)) - 6; // first sample of the next tile's row, seen from this lane's pair
    ue0 = c0p[d0]; ve0 = c0p[d0 + 8]; ue1 = c1p[d0]; ve1 = c1p[d0 + 8];
  }
  uint32_t pe[4], po[4];
  convert_quad(version, yw0, yw1, u0w, ue0, u1w, ue1, v0w, ve0, v1w, ve1, lastrow, lastcol, pe, po);
  if (active) {
    uint32_t *o = out + ((size_t)clip * height + y0) * width + x0;
    // written once, read by nobody on this GPU: past the caches (0.222 -> 0.215 ms per 512 clips of 640x480, A/B on one box)
    __builtin_nontemporal_store(u32x4{pe[0], pe[1], pe[2], pe[3]}, (u32x4 *)o);
    __builtin_nontemporal_store(u32x4{po[0], po[1], po[2], po[3]}, (u32x4 *)(o + width));
  }
}

extern "C" int mobi_launch_argb(const MobiReconArgs *a, int version, int clip0, int n_clips, uint32_t *out_dev, hipStream_t s) {
  if (n_clips <= 0) return 0;
  const int mbw = a->mbw, pairs = (mbw + 1) / 2;
  const dim3 grid((unsigned)(pairs * (a->n_mbs / mbw)), 1u, (unsigned)n_clips);
  hipLaunchKernelGGL(mobi_yuv_to_argb, grid, dim3(64), 0, s, (const uint8_t *)a->planes, (uint64_t)a->clip_bytes, a->slot_bytes, a->ring_base,
                     a->width, a->height, a->stride, version, clip0, out_dev);
  return (int)hipGetLastError();
}

// ---- self-test: div239 against the correctly rounded division for every float bit pattern ------------------
extern "C" __global__ void mobi_div239_check(unsigned long long *bad) {
  const uint32_t base = (blockIdx.x * 256u + threadIdx.x) * 256u;
  unsigned long long n = 0;
  for (uint32_t k = 0; k < 256; k++) {
    const float x = __uint_as_float(base + k);
    if (!(fabsf(x) >= 1e-30f && fabsf(x) <= 1e30f)) continue; // also drops NaN
    if (__float_as_uint(div239(x)) != __float_as_uint(__fdiv_rn(x, 239.0f))) n++;
  }
  if (n) atomicAdd(bad, n);
}
extern "C" long long mobi_launch_div239_check(hipStream_t s) {
  unsigned long long *bad = nullptr, h = 0;
  if (hipMalloc((void **)&bad, 8) != hipSuccess) return -1;
  (void)hipMemsetAsync(bad, 0, 8, s);
  hipLaunchKernelGGL(mobi_div239_check, dim3(65536), dim3(256), 0, s, bad);
  const bool ok = hipMemcpyAsync(&h, bad, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  (void)hipFree(bad);
  return ok ? (long long)h : -1;
}
