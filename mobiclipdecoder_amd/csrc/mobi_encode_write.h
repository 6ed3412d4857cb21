// mobi_encode_write.h -- stage 2 of the encoders, written once (device only): the scan of the macroblocks' bit lengths and the bit writer,
// with the frame's speller a parameter.  mobi_encode.hip instantiates them for I-frames (mobi_enc_scan, mobi_enc_write),
// mobi_encode_inter.hip for P-frames.
//
// A speller S knows one frame type's syntax over its launch arguments A (MobiEncArgs or a struct derived from it):
//   S::header_bits(A, pic)       the bits in front of the first macroblock
//   S::header(A, pic, put)       spells them
//   S::macroblock(A, pic, i, put) spells macroblock i (put(pattern, nbits), nbits <= 28)
//   S::total(A, pic, bits)       receives header + macroblock bits for the picture's statistics
// mobi_enc_scan_body: one workgroup of 256 per picture, exclusive scan of the bit lengths behind the header, the stream's length, whether
// it fits its slot.  mobi_enc_write_body: one lane per macroblock spells its bit string at its own offset into the zeroed slot: whole
// 32-bit words by plain stores, its first and last (shared with the neighbours) by atomic OR.
#ifndef MOBI_ENCODE_WRITE_H
#define MOBI_ENCODE_WRITE_H
#include <hip/hip_runtime.h>

#include "mobi_encode.h"

template <class S, class Args> __device__ __forceinline__ void mobi_enc_scan_body(const Args &A) {
  __shared__ uint32_t sh[256];
  const int pic = blockIdx.x, nmb = A.mbw * A.mbh, t = threadIdx.x;
  const MobiEncMb *mbs = A.mbs + (size_t)pic * nmb;
  uint32_t *off = A.mb_off + (size_t)pic * nmb;
  const uint32_t header = S::header_bits(A, pic);
  uint32_t carry = header;
  for (int base = 0; base < nmb; base += 256) {
    const int i = base + t;
    const uint32_t v = i < nmb ? mbs[i].bits : 0u;
    sh[t] = v;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
      const uint32_t a = t >= s ? sh[t - s] : 0u;
      __syncthreads();
      sh[t] += a;
      __syncthreads();
    }
    if (i < nmb) off[i] = carry + sh[t] - v;
    carry += sh[255];
    __syncthreads();
  }
  if (t == 0) {
    const uint64_t bytes = mobi_enc_stream_bytes_h(header, carry - header);
    A.bytes_out[pic] = (int32_t)bytes;
    A.fits[pic] = bytes <= A.slot_bytes;
    S::total(A, pic, carry);
  }
}

// MSB-first bits into 16-bit little-endian words, a 32-bit word (two of them) at a time
struct MobiEncSlotSink {
  uint32_t *slot;
  uint32_t pos, cur;
  bool first;
  __device__ void flush() {
    const uint32_t w = cur >> 16 | cur << 16;
    uint32_t *at = slot + ((pos - 1) >> 5);
    if (first) atomicOr(at, w); else *at = w;
    first = false;
    cur = 0;
  }
  __device__ void operator()(uint32_t v, int n) {
    const int b = (int)(pos & 31);
    if (b + n <= 32) {
      cur |= v << (32 - b - n);
      pos += n;
      if ((pos & 31) == 0) flush();
    } else {
      const int rest = b + n - 32;
      cur |= v >> rest;
      pos += n - rest;
      flush();
      cur = v << (32 - rest);
      pos += rest;
    }
  }
  __device__ void finish() {
    if (pos & 31) {
      pos = (pos + 31) & ~31u; // flush() addresses the word before pos
      first = true;            // the last word is shared with the next macroblock
      flush();
    }
  }
};

template <class S, class Args> __device__ __forceinline__ void mobi_enc_write_body(const Args &A) {
  const int pic = blockIdx.y, nmb = A.mbw * A.mbh, i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nmb || !A.fits[pic]) return;
  MobiEncSlotSink s;
  s.slot = (uint32_t *)(A.streams + (size_t)pic * A.slot_bytes);
  s.cur = 0;
  s.first = true;
  auto put = [&](uint32_t v, int n) { s(v, n); };
  if (i == 0) {
    s.pos = 0;
    S::header(A, pic, put);
  } else {
    s.pos = A.mb_off[(size_t)pic * nmb + i];
  }
  S::macroblock(A, pic, i, put);
  s.finish();
}

#endif
