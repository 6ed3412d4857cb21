// enc_parts_host_main.cpp -- TEST TOOL: the host model of the inter encoder's partition mode (mobi_encode_parts_host.cpp, i.e.
// csrc/mobi_encode_parts.h) as a stand-alone program, so that tests/test_encode_parts_model.py can run it under
// -fsanitize=address,undefined without loading anything into Python.
//   enc_parts_host_main W H version mode n in out   in:  n previous quantisers, n quantisers, n packed I420 pictures, n references
//                                                    out: n int32 lengths, then n slots of the mode's stream bound, then n reconstructions
// Exit 0, or 2 for bad usage / files, 3 when the model refuses or its written bits are not its priced bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/mobiclip_encode_parts.h"

struct MobiEncMb;
extern "C" size_t encq_host_bound(uint32_t width, uint32_t height, int mode);
extern "C" int encq_host_inter(uint32_t width, uint32_t height, int version, int mode, int n, const uint8_t *i420, size_t picture_pitch,
                               const uint8_t *ref_i420, size_t ref_pitch, const uint8_t *prev_quantizers, const uint8_t *quantizers, uint8_t *streams,
                               size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_inter_stats *stats, MobiEncMb *mbs, uint32_t *mv,
                               uint32_t *mvp, uint32_t *mv4, uint32_t *forms, int threads);

int main(int argc, char **argv) {
  if (argc != 8) return 2;
  const uint32_t W = (uint32_t)atoi(argv[1]), H = (uint32_t)atoi(argv[2]);
  const int version = atoi(argv[3]), mode = atoi(argv[4]), n = atoi(argv[5]);
  const size_t frame = (size_t)W * H * 3 / 2, slot = encq_host_bound(W, H, mode);
  if (n < 1 || !slot) return 2;
  // exact-size buffers: a read or write one byte outside a picture, a reference or a slot is the sanitizer's to report
  std::vector<uint8_t> pq(n), q(n), pics((size_t)n * frame), refs((size_t)n * frame), streams((size_t)n * slot), rec((size_t)n * frame);
  std::vector<int32_t> bytes(n);
  std::vector<mobi_enc_inter_stats> stats(n);
  FILE *f = fopen(argv[6], "rb");
  if (!f || fread(pq.data(), 1, pq.size(), f) != pq.size() || fread(q.data(), 1, q.size(), f) != q.size() ||
      fread(pics.data(), 1, pics.size(), f) != pics.size() || fread(refs.data(), 1, refs.size(), f) != refs.size())
    return 2;
  fclose(f);
  uint32_t forms[4] = {0, 0, 0, 0};
  if (encq_host_inter(W, H, version, mode, n, pics.data(), frame, refs.data(), frame, pq.data(), q.data(), streams.data(), slot, bytes.data(), rec.data(),
                      stats.data(), nullptr, nullptr, nullptr, nullptr, forms, 2) != 0)
    return 3;
  f = fopen(argv[7], "wb");
  if (!f || fwrite(bytes.data(), 4, bytes.size(), f) != bytes.size() || fwrite(streams.data(), 1, streams.size(), f) != streams.size() ||
      fwrite(rec.data(), 1, rec.size(), f) != rec.size())
    return 2;
  fclose(f);
  return 0;
}
