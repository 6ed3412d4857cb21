// enc_host_main.cpp -- TEST TOOL: the host model of the intra encoder (mobi_encode_host.cpp, i.e. csrc/mobi_encode.h) as a stand-alone
// program, so that tests/test_encode_model.py can run it under -fsanitize=address,undefined without loading anything into Python.
//   enc_host_main W H version n in out      in:  n quantiser bytes, then n packed I420 pictures
//                                           out: n int32 lengths, then n slots of the stream bound, then n reconstructions
// Exit 0, or 2 for bad usage / files, 3 when the model refuses or its written bits are not its priced bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/mobiclip_encode.h"

struct MobiEncMb;
extern "C" size_t enc_host_bound(uint32_t width, uint32_t height);
extern "C" int enc_host_intra(uint32_t width, uint32_t height, int version, int n, const uint8_t *i420, size_t picture_pitch, const uint8_t *quantizers,
                              int yuv_format, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, mobi_enc_stats *stats,
                              MobiEncMb *mbs, uint32_t *forms, int threads);

int main(int argc, char **argv) {
  if (argc != 7) return 2;
  const uint32_t W = (uint32_t)atoi(argv[1]), H = (uint32_t)atoi(argv[2]);
  const int version = atoi(argv[3]), n = atoi(argv[4]);
  const size_t frame = (size_t)W * H * 3 / 2, slot = enc_host_bound(W, H);
  if (n < 1 || !slot) return 2;
  std::vector<uint8_t> q(n), pics((size_t)n * frame), streams((size_t)n * slot), rec((size_t)n * frame);
  std::vector<int32_t> bytes(n);
  std::vector<mobi_enc_stats> stats(n);
  FILE *f = fopen(argv[5], "rb");
  if (!f || fread(q.data(), 1, q.size(), f) != q.size() || fread(pics.data(), 1, pics.size(), f) != pics.size()) return 2;
  fclose(f);
  uint32_t forms[4] = {0, 0, 0, 0};
  if (enc_host_intra(W, H, version, n, pics.data(), frame, q.data(), 0, streams.data(), slot, bytes.data(), rec.data(), stats.data(), nullptr, forms, 2) != 0)
    return 3;
  f = fopen(argv[6], "wb");
  if (!f || fwrite(bytes.data(), 4, bytes.size(), f) != bytes.size() || fwrite(streams.data(), 1, streams.size(), f) != streams.size() ||
      fwrite(rec.data(), 1, rec.size(), f) != rec.size())
    return 2;
  fclose(f);
  return 0;
}
