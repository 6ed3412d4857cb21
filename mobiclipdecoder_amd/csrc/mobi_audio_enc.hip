// mobi_audio_enc.hip -- the audio encoder's kernels for gfx950 (include/mobiclip_audio_enc.h; the rule: mobi_audio_enc.h).  Order exists
// only through kernel boundaries on the stream: the trial kernel leaves every (stream, channel)'s header index in device memory and the
// encode kernel, launched behind it, reads it.  No wave waits on a value in memory.
//
//   mobi_aenc_trials   one workgroup of 128 lanes per (stream, channel): block 0's 256 samples and the step table go to LDS once; lane i0
//                      < 89 codes the block from (x[0], i0) -- every lane reads the same LDS word, a broadcast -- and keeps E(i0) in 64
//                      bits; the (E, i0) keys are reduced to their minimum in LDS (ties to the smallest index ride in the key).
//   mobi_aenc_encode   ONE LANE per (stream, channel), as mobi_audio_blocks in the other direction: a workgroup is one wave, (64 / C) C of
//                      its lanes used.  Per quarter block the wave loads 64 rows of 64 samples into LDS with whole-row loads (row pitch 33
//                      dwords: lane i's dword k is in bank i + k), each lane codes its row -- the reconstruction replaces the input in
//                      place, the 32 nibble bytes go to a second LDS array of pitch 9 dwords (9 is odd: 64 lanes, 64 banks) -- and the
//                      wave writes the rows out: 8 lanes a row's 32 bytes into the slot, 64 lanes a row's 128 bytes of reconstruction.
//                      A lane stores itself only its header (the C headers of a stream are adjacent lanes' adjacent words), its 16 bytes
//                      of stats and, for channel 0, the stream's length.
//   mobi_aenc_pcm16    one thread per sample: the interleave.
#include <hip/hip_runtime.h>

#include "mobi_audio_enc.h"

namespace {

enum { kRowX = 33, kRowN = 9, kTrialLanes = 128 };

__global__ __launch_bounds__(kTrialLanes) void mobi_aenc_trials(const MobiAencArgs a) {
  __shared__ int16_t x[MOBI_AU_BLOCK_SAMPLES];
  __shared__ int16_t tab[96];
  __shared__ uint64_t key[kTrialLanes];
  const int tid = (int)threadIdx.x;
  const uint32_t g = blockIdx.x;
  const int16_t *src = a.samples + (uint64_t)g * a.sample_pitch;
  x[tid] = src[tid];
  x[tid + kTrialLanes] = src[tid + kTrialLanes];
  if (tid < 96) tab[tid] = a.step[tid];
  __syncthreads();
  uint64_t k = ~(uint64_t)0;
  if (tid < MOBI_AENC_INDICES) k = mobi_aenc_key(mobi_aenc_trial([&](int i) { return (int32_t)x[i]; }, MOBI_AU_BLOCK_SAMPLES, tid, tab), (uint32_t)tid);
  key[tid] = k;
  __syncthreads();
  for (int half = kTrialLanes / 2; half; half >>= 1) {
    if (tid < half) {
      const uint64_t o = key[tid + half];
      if (o < key[tid]) key[tid] = o;
    }
    __syncthreads();
  }
  if (tid == 0) a.start[g] = mobi_aenc_key_index(key[0]);
}

__global__ __launch_bounds__(64) void mobi_aenc_encode(const MobiAencArgs a) {
  __shared__ uint32_t xr[64 * kRowX]; // a row: 64 samples as 32 dwords, the input, then the reconstruction
  __shared__ uint32_t nb[64 * kRowN]; // a row: 32 nibble bytes as 8 dwords
  __shared__ int16_t tab[96];
  const int tid = (int)threadIdx.x, C = (int)a.n_channels, used = 64 / C * C;
  const uint32_t base = blockIdx.x * (uint32_t)used, g = base + tid;
  const bool live = tid < used && g < a.n_lanes;
  const uint32_t left = a.n_lanes - base, rows = left < (uint32_t)used ? left : (uint32_t)used; // the wave's live rows: 1 .. used
  for (int i = tid; i < 96; i += 64) tab[i] = a.step[i];

  MobiImaState st = {0, 0};
  MobiAencStats sum = {0, 0, 0};
  const uint32_t stream = g / (uint32_t)C, c = g % (uint32_t)C;
  if (live) {
    st.last = a.samples[(uint64_t)g * a.sample_pitch];
    st.index = (int32_t)a.start[g];
    sum.start_index = (uint32_t)st.index;
    *(uint32_t *)(a.slots + (uint64_t)stream * a.slot_pitch + MOBI_IMA_HEADER_BYTES * c) = ((uint32_t)st.index & 0xFFFFu) | ((uint32_t)st.last << 16);
    if (c == 0) a.sizes[stream] = (int32_t)mobi_aenc_frame_bytes(MOBI_AUDIO_IMA, (uint64_t)C, a.blocks);
  }
  int16_t *xr16 = (int16_t *)xr;
  uint32_t *mine = xr + tid * kRowX, *mine_n = nb + tid * kRowN;

  for (uint32_t b = 0; b < a.blocks; b++) {
#pragma unroll 1
    for (int sub = 0; sub < 4; sub++) {
      const uint64_t at = (uint64_t)b * MOBI_AU_BLOCK_SAMPLES + (uint64_t)sub * MOBI_AU_CHUNK;
      for (uint32_t r = 0; r < rows; r++) xr16[r * (2 * kRowX) + tid] = a.samples[(uint64_t)(base + r) * a.sample_pitch + at + tid];
      __syncthreads();
      if (live) {
#pragma unroll 1
        for (int j = 0; j < 8; j++) {
          uint32_t bytes = 0;
#pragma unroll
          for (int n = 0; n < 4; n++) {
            const uint32_t w = mine[4 * j + n];
            const int32_t x0 = (int16_t)(w & 0xFFFFu), x1 = (int16_t)(w >> 16);
            int32_t r0, r1;
            const uint32_t lo = mobi_aenc_sample(x0, st, tab, &r0, &sum.clamped);
            const uint32_t hi = mobi_aenc_sample(x1, st, tab, &r1, &sum.clamped);
            const int64_t d0 = (int64_t)x0 - r0, d1 = (int64_t)x1 - r1;
            sum.sse += (uint64_t)(d0 * d0) + (uint64_t)(d1 * d1);
            mine[4 * j + n] = ((uint32_t)r0 & 0xFFFFu) | ((uint32_t)r1 << 16);
            bytes |= (lo | hi << 4) << (8 * n);
          }
          mine_n[j] = bytes;
        }
      }
      __syncthreads();
      // nibble bytes: pass p writes the rows 8 p .. 8 p + 7, lane t dword t % 8 of row 8 p + t / 8
      for (uint32_t p = 0; p * 8 < rows; p++) {
        const uint32_t r = p * 8 + (uint32_t)tid / 8, k = (uint32_t)tid % 8;
        if (r < rows) {
          const uint32_t gr = base + r, s = gr / (uint32_t)C, ch = gr % (uint32_t)C;
          uint8_t *d = a.slots + (uint64_t)s * a.slot_pitch + mobi_aenc_block_offset((uint64_t)C, b, ch) + (uint64_t)sub * (MOBI_AU_CHUNK / 2);
          ((uint32_t *)d)[k] = nb[r * kRowN + k];
        }
      }
      if (a.recon)
        for (uint32_t r = 0; r < rows; r++) a.recon[(uint64_t)(base + r) * a.recon_pitch + at + tid] = xr16[r * (2 * kRowX) + tid];
      __syncthreads();
    }
  }
  if (live && a.stats) a.stats[g] = sum;
}

// element e of stream s = sample e / C of channel e % C
__global__ __launch_bounds__(256) void mobi_aenc_pcm16(const MobiAencArgs a, uint32_t blocks_per_stream) {
  const uint32_t s = blockIdx.x / blocks_per_stream, C = a.n_channels;
  const uint64_t e = (uint64_t)(blockIdx.x % blocks_per_stream) * 256 + threadIdx.x, S = (uint64_t)a.blocks * MOBI_AU_BLOCK_SAMPLES;
  if (e >= S * C) return;
  const uint64_t i = e / C, c = e % C, g = (uint64_t)s * C + c;
  const int16_t v = a.samples[g * a.sample_pitch + i];
  *(int16_t *)(a.slots + (uint64_t)s * a.slot_pitch + 2 * e) = v;
  if (a.recon) a.recon[g * a.recon_pitch + i] = v;
  if (i == 0 && a.stats) {
    const MobiAencStats none = {0, 0, 0};
    a.stats[g] = none;
  }
  if (e == 0) a.sizes[s] = (int32_t)mobi_aenc_frame_bytes(MOBI_AUDIO_PCM16, C, a.blocks);
}

} // namespace

#if defined(MOBI_PROFILING)
// profiling aid, in the profiling twin of the library only (tools/exp_audio_enc.py): which kernels an IMA call launches -- 0 both, 1 the
// trial kernel alone, 2 the encode kernel alone (it reads the indices an earlier call left)
static int g_only = 0;
extern "C" __attribute__((visibility("default"))) void mobi_debug_aenc_select(int only) { g_only = only; }
#define AENC_RUNS(k) (g_only == 0 || g_only == (k))
#else
#define AENC_RUNS(k) true
#endif

extern "C" int mobi_launch_audio_enc(const MobiAencArgs *a, hipStream_t s) {
  const uint32_t n_streams = a->n_lanes / a->n_channels;
  if (a->codec == MOBI_AUDIO_PCM16) {
    const uint64_t bps = ((uint64_t)a->blocks * MOBI_AU_BLOCK_SAMPLES * a->n_channels + 255) / 256;
    if (bps * n_streams > 0x7FFFFFFFull) return -1;
    mobi_aenc_pcm16<<<(unsigned)(bps * n_streams), 256, 0, s>>>(*a, (uint32_t)bps);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  if (AENC_RUNS(1)) mobi_aenc_trials<<<a->n_lanes, kTrialLanes, 0, s>>>(*a);
  if (hipGetLastError() != hipSuccess) return -1;
  const unsigned used = 64 / a->n_channels * a->n_channels;
  if (AENC_RUNS(2)) mobi_aenc_encode<<<(a->n_lanes + used - 1) / used, 64, 0, s>>>(*a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
