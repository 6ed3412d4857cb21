// enc_rate_host_main.cpp -- TEST TOOL: the host model of the rate rule (mobi_encode_rate_host.cpp, i.e. csrc/mobi_encode_rate.h over the
// three encoders' picture functions) as a stand-alone program, so that tests/test_encode_rate_model.py can run it under
// -fsanitize=address,undefined without loading anything into Python.
//   enc_rate_host_main W H version kind qmin qmax n in out
//       kind 0 (I-frames)            in:  n int32 targets, n packed I420 pictures
//       kind 1, 2 (P-frames, mode 0, 1) in:  n int32 targets, n previous quantisers, n pictures, n references
//       out: n chosen quantisers, n int32 lengths, then n slots of the kind's stream bound, then n reconstructions
// Exit 0, or 2 for bad usage / files, 3 when the model refuses or its written bits are not its priced bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" size_t encr_host_bound(uint32_t width, uint32_t height, int kind);
extern "C" int encr_host_target(uint32_t width, uint32_t height, int version, int kind, int n, const uint8_t *i420, size_t picture_pitch,
                                const uint8_t *ref_i420, size_t ref_pitch, const uint8_t *prev_quantizers, const int32_t *target_bytes, int qmin, int qmax,
                                int yuv_format, uint8_t *streams, size_t slot_bytes, int32_t *bytes_out, uint8_t *recon_i420, void *stats,
                                uint8_t *quantizers_out, int32_t *trials, int threads);

int main(int argc, char **argv) {
  if (argc != 10) return 2;
  const uint32_t W = (uint32_t)atoi(argv[1]), H = (uint32_t)atoi(argv[2]);
  const int version = atoi(argv[3]), kind = atoi(argv[4]), qmin = atoi(argv[5]), qmax = atoi(argv[6]), n = atoi(argv[7]);
  if (n < 1 || kind < 0 || kind > 2) return 2;
  const size_t frame = (size_t)W * H * 3 / 2, slot = encr_host_bound(W, H, kind);
  if (!slot) return 2;
  // exact-size buffers: a read or write one byte outside a picture, a reference, a slot or a row is the sanitizer's to report
  std::vector<int32_t> target(n), bytes(n);
  std::vector<uint8_t> pq(kind ? n : 0), pics((size_t)n * frame), refs(kind ? (size_t)n * frame : 0), streams((size_t)n * slot), rec((size_t)n * frame), qout(n);
  std::vector<uint64_t> stats((size_t)n * 8);
  FILE *f = fopen(argv[8], "rb");
  if (!f || fread(target.data(), 4, target.size(), f) != target.size() || fread(pq.data(), 1, pq.size(), f) != pq.size() ||
      fread(pics.data(), 1, pics.size(), f) != pics.size() || fread(refs.data(), 1, refs.size(), f) != refs.size())
    return 2;
  fclose(f);
  if (encr_host_target(W, H, version, kind, n, pics.data(), frame, kind ? refs.data() : nullptr, frame, kind ? pq.data() : nullptr, target.data(), qmin, qmax, 0,
                       streams.data(), slot, bytes.data(), rec.data(), stats.data(), qout.data(), nullptr, 2) != 0)
    return 3;
  f = fopen(argv[9], "wb");
  if (!f || fwrite(qout.data(), 1, qout.size(), f) != qout.size() || fwrite(bytes.data(), 4, bytes.size(), f) != bytes.size() ||
      fwrite(streams.data(), 1, streams.size(), f) != streams.size() || fwrite(rec.data(), 1, rec.size(), f) != rec.size())
    return 2;
  fclose(f);
  return 0;
}
