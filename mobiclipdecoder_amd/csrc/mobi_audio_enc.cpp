// mobi_audio_enc.cpp -- HOST: the entry points of include/mobiclip_audio_enc.h.  The object holds what it was made with and one device
// allocation (the IMA step table, then the header indices the trial kernel leaves for the encode kernel).  The _async call checks its
// arguments by the rule's own predicate (mobi_audio_enc.h), fills a MobiAencArgs and enqueues the kernels of mobi_audio_enc.hip: no
// allocation, no wait, no device value read here.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>

#include "mobi_audio_enc.h"

extern "C" int mobi_launch_audio_enc(const MobiAencArgs *a, hipStream_t s);

struct mobi_audio_enc {
  int device, codec, n_streams, n_channels, max_blocks;
  uint8_t *mem; // the one allocation: 96 int16 of the step table, then a uint32 per (stream, channel) at 256
};

extern "C" {

size_t mobi_audio_enc_frame_bytes(int codec, int n_channels, int blocks) {
  if (n_channels < 1 || n_channels > MOBI_AU_MAX_CHANNELS || blocks < 1) return 0;
  return (size_t)mobi_aenc_frame_bytes(codec, (uint64_t)n_channels, (uint64_t)blocks);
}

int mobi_audio_enc_check(int codec, int n_streams, int n_channels, int max_blocks, int n, const int16_t *samples, size_t sample_pitch, int blocks,
                         const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes, const int16_t *recon, size_t recon_pitch,
                         const void *stats) {
  return mobi_aenc_check_call(codec, n_streams, n_channels, max_blocks, n, samples, sample_pitch, blocks, slots, slot_pitch, slot_bytes, sizes, recon,
                              recon_pitch, stats);
}

mobi_audio_enc *mobi_audio_enc_create(int device, int codec, int n_streams, int n_channels, int max_blocks) {
  if (mobi_aenc_check_create(codec, n_streams, n_channels, max_blocks) != MOBI_OK) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  mobi_audio_enc *e = (mobi_audio_enc *)calloc(1, sizeof *e);
  if (!e) return nullptr;
  e->device = device;
  e->codec = codec;
  e->n_streams = n_streams;
  e->n_channels = n_channels;
  e->max_blocks = max_blocks;
  int16_t step[96] = {0};
  memcpy(step, mobi_ima_step, sizeof mobi_ima_step);
  if (hipMalloc((void **)&e->mem, 256 + (size_t)n_streams * n_channels * 4) != hipSuccess ||
      hipMemcpy(e->mem, step, sizeof step, hipMemcpyHostToDevice) != hipSuccess) {
    if (e->mem) (void)hipFree(e->mem);
    free(e);
    return nullptr;
  }
  return e;
}

void mobi_audio_enc_destroy(mobi_audio_enc *e) {
  if (!e) return;
  if (e->mem) (void)hipFree(e->mem);
  free(e);
}

int mobi_audio_enc_async(mobi_audio_enc *e, void *stream, int n, const int16_t *samples, size_t sample_pitch, int blocks, uint8_t *slots,
                         size_t slot_pitch, size_t slot_bytes, int32_t *sizes, int16_t *recon, size_t recon_pitch, mobi_audio_enc_stats *stats) {
  if (!e) return MOBI_E_ARG;
  const int rc = mobi_aenc_check_call(e->codec, e->n_streams, e->n_channels, e->max_blocks, n, samples, sample_pitch, blocks, slots, slot_pitch, slot_bytes,
                                      sizes, recon, recon_pitch, stats);
  if (rc != MOBI_OK) return rc;
  if (hipSetDevice(e->device) != hipSuccess) return MOBI_E_DEVICE;
  MobiAencArgs a;
  memset(&a, 0, sizeof a);
  a.step = (const int16_t *)e->mem;
  a.start = (uint32_t *)(e->mem + 256);
  a.samples = samples;
  a.sample_pitch = sample_pitch;
  a.slots = slots;
  a.slot_pitch = slot_pitch;
  a.sizes = sizes;
  a.recon = recon;
  a.recon_pitch = recon_pitch;
  a.stats = (MobiAencStats *)stats;
  a.n_lanes = (uint32_t)n * (uint32_t)e->n_channels;
  a.n_channels = (uint32_t)e->n_channels;
  a.blocks = (uint32_t)blocks;
  a.codec = e->codec;
  return mobi_launch_audio_enc(&a, (hipStream_t)stream) == 0 ? MOBI_OK : MOBI_E_DEVICE;
}

} // extern "C"
