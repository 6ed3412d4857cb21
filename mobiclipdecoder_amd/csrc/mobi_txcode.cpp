// mobi_txcode.cpp -- the C entry points of the encoder's transform coding (include/mobiclip_hip.h: mobi_encoder_qtables,
// mobi_transform_code, mobi_transform_code_async) and the per-device constants of the kernel (mobi_txcode.hip).
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mobiclip_hip.h"
#include "mobi_txcode.h"

extern "C" int mobi_launch_txcode(int n, const MobiTcArgs *a, hipStream_t s);

namespace {

// Q rows, reciprocals, scan orders and the cost table: built and uploaded once per device, at its first call; never freed (a few KB)
std::mutex g_const_mutex;
std::vector<MobiTcConst *> g_const;

MobiTcConst *device_const(int device) {
  std::lock_guard<std::mutex> l(g_const_mutex);
  if ((size_t)device < g_const.size() && g_const[device]) return g_const[device];
  MobiTcConst h;
  mobi_tc_build_const(&h);
  MobiTcConst *d = nullptr;
  if (hipMalloc((void **)&d, sizeof h) != hipSuccess) return nullptr;
  if (hipMemcpy(d, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return nullptr;
  }
  if (g_const.size() <= (size_t)device) g_const.resize(device + 1, nullptr);
  return g_const[device] = d;
}

// the argument checks both entry points share (MOBI_E_ARG), then the launch arguments except the buffers
int check_args(int device, int n, const int *quantizers, int n_q, const void *src, const void *pred, size_t n_blocks, const void *bits_out,
               const void *flags_out, MobiTcArgs *a) {
  if (device < 0 || (n != 4 && n != 8) || n_q < 1 || n_q > MOBI_TC_NQ || !quantizers) return MOBI_E_ARG;
  for (int i = 0; i < n_q; i++)
    if (quantizers[i] < 0 || quantizers[i] >= MOBI_TC_NQ) return MOBI_E_ARG;
  if (n_blocks && (!src || !pred || !bits_out || !flags_out)) return MOBI_E_ARG;
  // block and entry indices are 32-bit in the kernel (entry e = qi * n_blocks + b)
  if (n_blocks > 0xFFFFFFFFull / (uint64_t)n_q) return MOBI_E_ARG;
  memset(a, 0, sizeof *a);
  a->n_blocks = (uint32_t)n_blocks;
  a->n_q = n_q;
  for (int i = 0; i < n_q; i++) a->q[i] = (uint8_t)quantizers[i];
  return MOBI_OK;
}

} // namespace

int mobi_encoder_qtables(int quantizer, float *qtable4x4, float *qtable8x8) {
  if (quantizer < 0 || quantizer >= MOBI_TC_NQ) return MOBI_E_ARG;
  int32_t t[64];
  if (qtable4x4) {
    mobi_tc_qtable(quantizer, 4, t);
    for (int i = 0; i < 16; i++) qtable4x4[i] = (float)t[i];
  }
  if (qtable8x8) {
    mobi_tc_qtable(quantizer, 8, t);
    for (int i = 0; i < 64; i++) qtable8x8[i] = (float)t[i];
  }
  return MOBI_OK;
}

int mobi_transform_code_async(int device, void *stream, int n, const int *quantizers, int n_q, const uint8_t *src, const uint8_t *pred,
                              size_t n_blocks, int16_t *levels_out, uint8_t *recon_out, int32_t *bits_out, int32_t *sad_out, uint8_t *flags_out) {
  MobiTcArgs a;
  const int rc = check_args(device, n, quantizers, n_q, src, pred, n_blocks, bits_out, flags_out, &a);
  if (rc != MOBI_OK || n_blocks == 0) return rc;
  if (hipSetDevice(device) != hipSuccess) return MOBI_E_DEVICE;
  if (!(a.k = device_const(device))) return MOBI_E_DEVICE;
  a.src = src;
  a.pred = pred;
  a.levels = levels_out;
  a.recon = recon_out;
  a.bits = bits_out;
  a.sad = sad_out;
  a.flags = flags_out;
  return mobi_launch_txcode(n, &a, (hipStream_t)stream) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

int mobi_transform_code(int device, int n, const int *quantizers, int n_q, const uint8_t *src, const uint8_t *pred, size_t n_blocks,
                        int16_t *levels_out, uint8_t *recon_out, int32_t *bits_out, int32_t *sad_out, uint8_t *flags_out) {
  MobiTcArgs a;
  int rc = check_args(device, n, quantizers, n_q, src, pred, n_blocks, bits_out, flags_out, &a);
  if (rc != MOBI_OK || n_blocks == 0) return rc;
  if (hipSetDevice(device) != hipSuccess) return MOBI_E_DEVICE;
  const size_t nn = (size_t)n * n, in_bytes = n_blocks * nn, entries = n_blocks * (size_t)n_q;
  // one device allocation, carved: src, pred, levels, recon, bits, sad, flags (each part 256-byte aligned)
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_pred = up(in_bytes), o_lev = o_pred + up(in_bytes), o_rec = o_lev + (levels_out ? up(entries * nn * 2) : 0),
               o_bits = o_rec + (recon_out ? up(entries * nn) : 0), o_sad = o_bits + up(entries * 4),
               o_flags = o_sad + (sad_out ? up(entries * 4) : 0), total = o_flags + up(entries);
  uint8_t *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) return MOBI_E_DEVICE;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    (void)hipFree(d);
    return MOBI_E_DEVICE;
  }
  rc = hipMemcpyAsync(d, src, in_bytes, hipMemcpyHostToDevice, s) == hipSuccess && hipMemcpyAsync(d + o_pred, pred, in_bytes, hipMemcpyHostToDevice, s) == hipSuccess
           ? mobi_transform_code_async(device, s, n, quantizers, n_q, d, d + o_pred, n_blocks, levels_out ? (int16_t *)(d + o_lev) : nullptr,
                                       recon_out ? d + o_rec : nullptr, (int32_t *)(d + o_bits), sad_out ? (int32_t *)(d + o_sad) : nullptr, d + o_flags)
           : MOBI_E_DEVICE;
  if (rc == MOBI_OK &&
      ((levels_out && hipMemcpyAsync(levels_out, d + o_lev, entries * nn * 2, hipMemcpyDeviceToHost, s) != hipSuccess) ||
       (recon_out && hipMemcpyAsync(recon_out, d + o_rec, entries * nn, hipMemcpyDeviceToHost, s) != hipSuccess) ||
       hipMemcpyAsync(bits_out, d + o_bits, entries * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
       (sad_out && hipMemcpyAsync(sad_out, d + o_sad, entries * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
       hipMemcpyAsync(flags_out, d + o_flags, entries, hipMemcpyDeviceToHost, s) != hipSuccess))
    rc = MOBI_E_DEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = MOBI_E_DEVICE;
  (void)hipStreamDestroy(s);
  (void)hipFree(d);
  return rc;
}
