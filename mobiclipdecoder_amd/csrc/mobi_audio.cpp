// mobi_audio.cpp -- the device side's C entry points of the batched audio decode (include/mobiclip_audio.h): the handle, and
// mobi_audio_decode: plan every stream (mobi_audio_plan.cpp), gather the audio bytes into pinned staging, one copy, one launch
// (mobi_audio.hip).  The decoder states live in device memory; what the host keeps per stream is what the framing needs to plan the next
// frame: the Mods channel cursor, which IMA decoders are new, and which streams were reset since the last launch.
// Sx (include/mobiclip_sx.h, mobi_sx.hip) shares the handle and the call: its packets have their own lengths, its lanes their codebooks in
// device memory, and a stream refilled by mobi_sx_reset gets its new codebooks behind the packets of the next call's one copy.
#include "../../include/mobiclip_audio.h"
#include "../../include/mobiclip_sx.h"
#include "mobi_audio.h"
#include "mobi_batch.h"
#include "mobi_sx.h"

extern "C" int mobi_launch_audio(const MobiAudioArgs *a, hipStream_t s);
extern "C" int mobi_launch_sx(const MobiAudioArgs *a, const uint8_t *books, hipStream_t s);
bool mobi_audio_args_ok(int framing, int codec, int n_channels); // mobi_audio_plan.cpp

namespace {

int s16le(const uint8_t *p) { return (int16_t)(uint16_t)(p[0] | (p[1] << 8)); }

// the tables as the kernels read them: built once per device, at its first handle; never freed (1.5 KB)
std::mutex g_const_mutex;
std::vector<MobiAudioConst *> g_const;

template <size_t N, size_t M> void fill(int16_t (&dst)[N], const int16_t (&src)[M]) {
  static_assert(M <= N, "table");
  memset(dst, 0, sizeof dst);
  memcpy(dst, src, sizeof src);
}

MobiAudioConst *device_const(int device) {
  std::lock_guard<std::mutex> l(g_const_mutex);
  if ((size_t)device < g_const.size() && g_const[device]) return g_const[device];
  MobiAudioConst h;
  fill(h.pulse, mobi_fa_pulse);
  fill(h.step, mobi_ima_step);
  fill(h.k01, mobi_fa_k01);
  fill(h.k2, mobi_fa_k2);
  fill(h.k3, mobi_fa_k3);
  fill(h.k4, mobi_fa_k4);
  fill(h.k5, mobi_fa_k5);
  fill(h.k6, mobi_fa_k6);
  fill(h.k7, mobi_fa_k7);
  MobiAudioConst *d = nullptr;
  if (hipMalloc((void **)&d, sizeof h) != hipSuccess) return nullptr;
  if (hipMemcpy(d, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return nullptr;
  }
  if (g_const.size() <= (size_t)device) g_const.resize(device + 1, nullptr);
  return g_const[device] = d;
}

} // namespace

struct mobi_audio {
  int device = 0, framing = 0, codec = 0, n_streams = 0, C = 0;
  std::mutex mutex;
  std::vector<int> cursor;    // [n_streams]: Mods, the channel of the next packet
  std::vector<uint8_t> fresh; // [n_streams * C]: IMA in Mods framing, the channel's decoder is new (its next packet carries the header)
  std::vector<uint8_t> zero;  // [n_streams]: reset since the last launch: the kernel zeroes the states first
  MobiAudioConst *k = nullptr;
  DevArr<int32_t> state;      // [MOBI_AU_STATE_WORDS][n_streams * C]; Sx: [MOBI_SX_STATE_WORDS][n_streams * C]
  DevArr<uint8_t> books;      // Sx: [n_streams * C][MOBI_SX_BOOK_PITCH], the codebooks as the kernel reads them
  std::vector<uint8_t> pend;  // Sx: [n_streams * C][MOBI_SX_BOOK_PITCH], codebooks of mobi_sx_reset that the next launch's copy takes along
  std::vector<uint8_t> has_pend; // Sx: [n_streams]
  // two staging pairs: while the kernel of one call reads dev[i], the next call fills pin[i ^ 1]; ev[i] = the end of the kernel that read dev[i]
  PinnedBuf pin[2];
  DevBuf dev[2];
  Event ev[2];
  bool busy[2] = {false, false};
  int turn = 0;
  // the plan of the call in progress (kept between calls: no allocation once the sizes have been seen)
  std::vector<mobi_audio_block> blocks;
  std::vector<size_t> first, count;   // [n_streams]: the stream's blocks in `blocks`
  std::vector<int> new_cursor;        // [n_streams]
  std::vector<uint32_t> lane_blocks;  // [n_streams * C]
  std::vector<uint32_t> lane_fill;    // [n_streams * C]: blocks gathered so far (Sx: bytes)
  std::vector<uint32_t> lane_bytes;   // Sx: [n_streams * C], the bytes of the lane's packets
};

// codebooks == nullptr: every codec but Sx
static mobi_audio *audio_create(int device, int framing, int codec, int n_streams, int n_channels, const uint8_t *const *codebooks) {
  if (device < 0 || !mobi_audio_args_ok(framing, codec, n_channels) || (codec == MOBI_AUDIO_SX) != (codebooks != nullptr) || n_streams < 1 ||
      (int64_t)n_streams * n_channels >= (1 << 24))
    return nullptr;
  if (codebooks)
    for (int64_t g = 0; g < (int64_t)n_streams * n_channels; g++)
      if (!codebooks[g]) return nullptr;
  if (hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  std::unique_ptr<mobi_audio> a(new mobi_audio);
  a->device = device, a->framing = framing, a->codec = codec, a->n_streams = n_streams, a->C = n_channels;
  const size_t lanes = (size_t)n_streams * n_channels;
  a->cursor.assign(n_streams, 0);
  a->fresh.assign(lanes, 1);
  a->zero.assign(n_streams, 1); // the first launch zeroes the states on its own stream, as one after a reset does
  a->first.resize(n_streams), a->count.resize(n_streams), a->new_cursor.resize(n_streams);
  a->lane_blocks.resize(lanes), a->lane_fill.resize(lanes);
  if (codebooks) {
    a->lane_bytes.resize(lanes);
    a->has_pend.assign(n_streams, 0);
    std::vector<uint8_t> h(lanes * MOBI_SX_BOOK_PITCH, 0);
    for (size_t g = 0; g < lanes; g++) memcpy(h.data() + g * MOBI_SX_BOOK_PITCH, codebooks[g], MOBI_SX_CODEBOOK);
    if (a->books.alloc(h.size()) != MOBI_OK || hipMemcpy(a->books, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
  } else if (!(a->k = device_const(device))) return nullptr;
  if (a->state.alloc(lanes * (codebooks ? (size_t)MOBI_SX_STATE_WORDS : (size_t)MOBI_AU_STATE_WORDS)) != MOBI_OK) return nullptr;
  for (auto &e : a->ev)
    if (ensure_event(e) != MOBI_OK) return nullptr;
  return a.release();
}

mobi_audio *mobi_audio_create(int device, int framing, int codec, int n_streams, int n_channels) {
  return codec == MOBI_AUDIO_SX ? nullptr : audio_create(device, framing, codec, n_streams, n_channels, nullptr); // Sx: mobi_sx_create
}

mobi_audio *mobi_sx_create(int device, int n_streams, int n_channels, const uint8_t *const *codebooks) {
  return codebooks ? audio_create(device, MOBI_AUDIO_FRAMING_MODS, MOBI_AUDIO_SX, n_streams, n_channels, codebooks) : nullptr;
}

void mobi_audio_destroy(mobi_audio *a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  for (int i = 0; i < 2; i++)
    if (a->busy[i]) (void)hipEventSynchronize(a->ev[i]); // the kernels still read the staging buffers and write the states
  delete a;
}

int mobi_audio_reset(mobi_audio *a, const int32_t *streams, int count, int keep_cursor) {
  if (!a || count < 0 || (count && !streams)) return MOBI_E_ARG;
  for (int i = 0; i < count; i++)
    if (streams[i] < 0 || streams[i] >= a->n_streams) return MOBI_E_ARG;
  std::lock_guard<std::mutex> l(a->mutex);
  for (int i = 0; i < count; i++) {
    const int s = streams[i];
    a->zero[s] = 1;
    for (int c = 0; c < a->C; c++) a->fresh[(size_t)s * a->C + c] = 1;
    if (!keep_cursor) a->cursor[s] = 0;
  }
  return MOBI_OK;
}

int mobi_sx_reset(mobi_audio *a, const int32_t *streams, int count, const uint8_t *const *codebooks) {
  if (!a || a->codec != MOBI_AUDIO_SX || count < 0 || (count && (!streams || !codebooks))) return MOBI_E_ARG;
  for (int i = 0; i < count; i++) {
    if (streams[i] < 0 || streams[i] >= a->n_streams) return MOBI_E_ARG;
    for (int c = 0; c < a->C; c++)
      if (!codebooks[(size_t)i * a->C + c]) return MOBI_E_ARG;
  }
  std::lock_guard<std::mutex> l(a->mutex);
  if (count && a->pend.empty()) a->pend.assign((size_t)a->n_streams * a->C * MOBI_SX_BOOK_PITCH, 0);
  for (int i = 0; i < count; i++) {
    const int s = streams[i];
    a->zero[s] = 1, a->has_pend[s] = 1, a->cursor[s] = 0;
    for (int c = 0; c < a->C; c++) memcpy(&a->pend[((size_t)s * a->C + c) * MOBI_SX_BOOK_PITCH], codebooks[(size_t)i * a->C + c], MOBI_SX_CODEBOOK);
  }
  return MOBI_OK;
}

int mobi_audio_decode(mobi_audio *a, void *stream, const uint8_t *const *data, const size_t *len, const size_t *offsets,
                      const uint32_t *n_packets, int dtype, int layout, void *dst, size_t dst_bytes, size_t max_samples,
                      int32_t *n_samples_out, int *rc) {
  if (!a || !data || !len || !dst || !n_samples_out || !rc) return MOBI_E_ARG;
  const bool mods = a->framing == MOBI_AUDIO_FRAMING_MODS, pcm = a->codec == MOBI_AUDIO_PCM16, sx = a->codec == MOBI_AUDIO_SX;
  if (mods && (!offsets || !n_packets)) return MOBI_E_ARG;
  if ((dtype != MOBI_AUDIO_S16 && dtype != MOBI_AUDIO_F32) || (layout != MOBI_AUDIO_PLANAR && layout != MOBI_AUDIO_INTERLEAVED)) return MOBI_E_ARG;
  const int S = a->n_streams, C = a->C;
  const size_t lanes = (size_t)S * C, elem = dtype == MOBI_AUDIO_F32 ? 4 : 2;
  if (max_samples > 0x7FFFFFFF || lanes * max_samples > dst_bytes / elem || ((uintptr_t)dst & (elem - 1))) return MOBI_E_ARG;
  std::lock_guard<std::mutex> l(a->mutex);

  // ---- plan every stream; nothing of the handle changes before the whole call is known to be good ----
  const size_t blk = sx ? 10 /* the shortest packet */ : a->codec == MOBI_AUDIO_FASTAUDIO ? MOBI_FA_BLOCK_BYTES : MOBI_IMA_BLOCK_BYTES;
  const uint32_t block_samples = sx ? MOBI_SX_SAMPLES : MOBI_AU_BLOCK_SAMPLES;
  size_t bound = 0;
  for (int s = 0; s < S; s++) {
    if (!data[s] && len[s]) return MOBI_E_ARG;
    if (!pcm && len[s]) bound += mods ? std::min<size_t>(n_packets[s], len[s] / blk) : len[s] / blk; // no more blocks than fit: a garbage count is the plan's MOBI_E_INDEX
  }
  if (a->blocks.size() < bound) a->blocks.resize(bound);
  size_t total_blocks = 0, pcm_bytes = 0;
  uint32_t pcm_max = 0;
  bool any_zero = false;
  for (int s = 0; s < S; s++) {
    int cur = a->cursor[s];
    size_t n = 0;
    int32_t *ns = n_samples_out + (size_t)s * C;
    rc[s] = sx ? mobi_sx_plan(C, data[s], len[s], offsets[s], n_packets[s], &cur, a->blocks.data() + total_blocks, bound - total_blocks, &n, ns)
               : mobi_audio_plan(a->framing, a->codec, C, data[s], len[s], mods ? offsets[s] : 0, mods ? n_packets[s] : 0, &cur,
                                 &a->fresh[(size_t)s * C], a->blocks.data() + total_blocks, bound - total_blocks, &n, ns);
    if (rc[s] != MOBI_OK && rc[s] != MOBI_E_INDEX) return rc[s];
    a->first[s] = total_blocks, a->count[s] = n, a->new_cursor[s] = cur;
    total_blocks += n;
    for (int c = 0; c < C; c++) {
      if ((size_t)ns[c] > max_samples) return MOBI_E_ARG;
      if (layout == MOBI_AUDIO_INTERLEAVED && ns[c] != ns[0]) return MOBI_E_ARG;
      a->lane_blocks[(size_t)s * C + c] = (uint32_t)ns[c] / block_samples;
      if (!pcm && a->lane_blocks[(size_t)s * C + c] > 0xFFFF) return MOBI_E_ARG;
      if (sx) a->lane_bytes[(size_t)s * C + c] = 0;
    }
    if (sx) // a packet's length is in its second word (the plan has checked that it fits)
      for (size_t i = 0; i < n; i++) {
        const mobi_audio_block &b = a->blocks[a->first[s] + i];
        a->lane_bytes[(size_t)s * C + b.channel] += (uint32_t)mobi_sx_packet_bytes((uint32_t)data[s][b.offset + 3] << 8);
      }
    if (pcm) {
      pcm_bytes += align_up((size_t)ns[0] * 2 * C, kAlign);
      pcm_max = std::max(pcm_max, (uint32_t)ns[0]);
    }
    any_zero |= a->zero[s] != 0;
  }
  if (pcm ? pcm_max == 0 : (total_blocks == 0 && !any_zero)) return MOBI_OK; // nothing to enqueue

  // ---- the staged bytes: [one MobiAudioLane per lane (PCM16: per stream)][every lane's blocks back to back, each lane on 16 bytes]
  //      [Sx: the codebooks of the streams mobi_sx_reset refilled, MOBI_SX_BOOK_PITCH each] ----
  const size_t n_desc = pcm ? (size_t)S : lanes, head = align_up(n_desc * sizeof(MobiAudioLane), kAlign);
  auto lane_size = [&](size_t g) { return sx ? (size_t)a->lane_bytes[g] : a->lane_blocks[g] * blk; };
  size_t total = head + pcm_bytes;
  if (!pcm)
    for (size_t g = 0; g < lanes; g++) total += align_up(lane_size(g), kAlign);
  if (total - head > 0xFFFFFFFFull) return MOBI_E_ARG;
  const size_t books_at = total;
  if (sx)
    for (int s = 0; s < S; s++)
      if (a->has_pend[s]) total += (size_t)C * MOBI_SX_BOOK_PITCH;

  HIP_TRY(hipSetDevice(a->device));
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, dst) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if (at.type != hipMemoryTypeDevice || at.device != a->device) return MOBI_E_ARG;
  hipDeviceptr_t abase = nullptr;
  size_t arange = 0;
  if (hipMemGetAddressRange(&abase, &arange, (hipDeviceptr_t)dst) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if ((uintptr_t)dst + lanes * max_samples * elem > (uintptr_t)abase + arange) return MOBI_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); return MOBI_E_ARG; }
  if (cap != hipStreamCaptureStatusNone) return MOBI_E_ARG;

  const int t = a->turn;
  if (a->busy[t]) HIP_TRY(hipEventSynchronize(a->ev[t])); // the kernel of the call before the previous one: never this call's own
  a->busy[t] = false;
  // the states are one device array that successive kernels read and write: behind the previous call's kernel, whatever stream that was on
  if (a->busy[t ^ 1]) HIP_TRY(hipStreamWaitEvent(st, a->ev[t ^ 1], 0));
  if (int e = a->pin[t].reserve(total)) return e;
  if (int e = a->dev[t].reserve(total)) return e;
  uint8_t *h = a->pin[t].p;
  MobiAudioLane *desc = (MobiAudioLane *)h;
  memset(desc, 0, head);
  size_t at_byte = 0;
  if (pcm) {
    for (int s = 0; s < S; s++) {
      const size_t n = (size_t)n_samples_out[(size_t)s * C] * 2 * C;
      desc[s].off = (uint32_t)at_byte;
      desc[s].n_pcm = (uint32_t)n_samples_out[(size_t)s * C];
      if (n) memcpy(h + head + at_byte, data[s], n);
      at_byte += align_up(n, kAlign);
    }
  } else {
    for (size_t g = 0; g < lanes; g++) {
      desc[g].off = (uint32_t)at_byte;
      desc[g].nblk = (uint16_t)a->lane_blocks[g];
      desc[g].flags = a->zero[g / C] ? MOBI_AU_ZERO : 0;
      a->lane_fill[g] = 0;
      at_byte += align_up(lane_size(g), kAlign);
    }
    for (int s = 0; s < S; s++) {
      const mobi_audio_block *b = a->blocks.data() + a->first[s];
      for (size_t i = 0; i < a->count[s]; i++) {
        const size_t g = (size_t)s * C + b[i].channel;
        if (b[i].header) {
          desc[g].flags |= MOBI_AU_HEADER;
          desc[g].hdr_index = (uint8_t)(s16le(data[s] + b[i].header_offset) & 0x7F);
          desc[g].hdr_last = s16le(data[s] + b[i].header_offset + 2);
        }
        if (sx) {
          const size_t n = (size_t)mobi_sx_packet_bytes((uint32_t)data[s][b[i].offset + 3] << 8);
          memcpy(h + head + desc[g].off + a->lane_fill[g], data[s] + b[i].offset, n);
          a->lane_fill[g] += (uint32_t)n;
        } else
          memcpy(h + head + desc[g].off + a->lane_fill[g]++ * blk, data[s] + b[i].offset, blk);
      }
    }
  }
  if (sx) {
    size_t at = books_at;
    for (int s = 0; s < S; s++)
      if (a->has_pend[s]) {
        memcpy(h + at, &a->pend[(size_t)s * C * MOBI_SX_BOOK_PITCH], (size_t)C * MOBI_SX_BOOK_PITCH);
        at += (size_t)C * MOBI_SX_BOOK_PITCH;
      }
  }

  HIP_TRY(hipMemcpyAsync(a->dev[t].p, h, total, hipMemcpyHostToDevice, st));
  a->busy[t] = true; // from here on the buffers are in use, whatever follows
  if (sx) {
    size_t at = books_at;
    for (int s = 0; s < S; s++)
      if (a->has_pend[s]) {
        HIP_TRY(hipMemcpyAsync(a->books + (size_t)s * C * MOBI_SX_BOOK_PITCH, a->dev[t].p + at, (size_t)C * MOBI_SX_BOOK_PITCH, hipMemcpyDeviceToDevice, st));
        at += (size_t)C * MOBI_SX_BOOK_PITCH;
      }
  }
  MobiAudioArgs k;
  memset(&k, 0, sizeof k);
  k.k = a->k;
  k.lanes = (const MobiAudioLane *)a->dev[t].p;
  k.data = a->dev[t].p + head;
  k.state = a->state;
  k.dst = dst;
  k.max_samples = max_samples;
  k.n_lanes = (uint32_t)n_desc;
  k.n_channels = (uint32_t)C;
  k.pcm_max = pcm_max;
  k.codec = a->codec, k.dtype = dtype, k.layout = layout;
  const int launched = sx ? mobi_launch_sx(&k, a->books, st) : mobi_launch_audio(&k, st);
  HIP_TRY(hipEventRecord(a->ev[t], st));
  a->turn = t ^ 1;
  if (launched != 0) return MOBI_E_DEVICE;

  // ---- the call is enqueued: the framing state moves on for the streams that decoded ----
  for (int s = 0; s < S; s++) {
    a->zero[s] = 0;
    if (sx) a->has_pend[s] = 0;
    if (rc[s] != MOBI_OK) continue;
    a->cursor[s] = a->new_cursor[s];
    for (int c = 0; c < C; c++)
      if (a->lane_blocks[(size_t)s * C + c]) a->fresh[(size_t)s * C + c] = 0;
  }
  return MOBI_OK;
}
