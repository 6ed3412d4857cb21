// mux_host_main.cpp -- TEST TOOL: the host model of the muxing rule (mobi_mux_host.cpp, i.e. csrc/mobi_mux.h) as a stand-alone program,
// so that tests/test_mux_model.py can run it under -fsanitize=address,undefined without loading anything into Python.
//   mux_host_main container width height max_keys n T capacity slot_bytes in out
//       in:  T x n int32 lengths, T key flags (bytes), T x n slots of slot_bytes
//       out: n int64 file lengths, n int32 status words, n rows of capacity bytes (0xA5 where nothing was written)
// Exit 0, or 2 for bad usage / files, 3 when the model refuses.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int mux_host_run(int container, uint32_t width, uint32_t height, uint32_t fps_rate, uint32_t fps_scale, uint32_t fps_raw, int max_keys, int n, int T,
                            uint8_t *files, size_t pitch, size_t capacity, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes, const int32_t *sizes,
                            const uint8_t *key_flags, int64_t *bytes_out, int32_t *status_out);

int main(int argc, char **argv) {
  if (argc != 11) return 2;
  const int container = atoi(argv[1]), max_keys = atoi(argv[4]), n = atoi(argv[5]), T = atoi(argv[6]);
  const uint32_t W = (uint32_t)atoi(argv[2]), H = (uint32_t)atoi(argv[3]);
  const size_t capacity = (size_t)atoll(argv[7]), slot = (size_t)atoll(argv[8]);
  if (n < 1 || T < 1 || !slot) return 2;
  // exact-size buffers: a read one byte outside a slot or a row of lengths, a write one byte outside the n capacities is the sanitizer's
  // to report (the rows lie back to back: pitch == capacity)
  std::vector<int32_t> sizes((size_t)T * n), status(n);
  std::vector<uint8_t> keys(T), slots((size_t)T * n * slot), files((size_t)n * capacity, 0xA5);
  std::vector<int64_t> bytes(n);
  FILE *f = fopen(argv[9], "rb");
  if (!f || fread(sizes.data(), 4, sizes.size(), f) != sizes.size() || fread(keys.data(), 1, keys.size(), f) != keys.size() ||
      fread(slots.data(), 1, slots.size(), f) != slots.size())
    return 2;
  fclose(f);
  if (mux_host_run(container, W, H, 30, 1, 0x18000000, max_keys, n, T, files.data(), capacity, capacity, slots.data(), slot, slot, sizes.data(), keys.data(),
                   bytes.data(), status.data()) != 0)
    return 3;
  f = fopen(argv[10], "wb");
  if (!f || fwrite(bytes.data(), 8, bytes.size(), f) != bytes.size() || fwrite(status.data(), 4, status.size(), f) != status.size() ||
      fwrite(files.data(), 1, files.size(), f) != files.size())
    return 2;
  fclose(f);
  return 0;
}
