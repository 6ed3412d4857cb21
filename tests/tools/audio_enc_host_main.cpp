// audio_enc_host_main.cpp -- TEST TOOL: the host models of the audio encoder (mobi_audio_enc_host.cpp, i.e. csrc/mobi_audio_enc.h) and of
// the muxer with an audio stream (mobi_mux_audio_host.cpp, i.e. csrc/mobi_mux.h) as a stand-alone program, so that
// tests/test_audio_enc_model.py can run them under -fsanitize=address,undefined without loading anything into Python.
//   audio_enc_host_main codec n C B in out
//       in:  n x C x 256 B int16 samples
//       out: n frames back to back, n x C x 256 B int16 of reconstruction, n x C stats of 16 bytes, then the Moflex file of ONE clip
//            that carries the n frames, in order, as the frames of its audio stream
// Exit 0, or 2 for bad usage / files, 3 when a model refuses.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int aenc_host_run(int codec, int n_streams, int C, int max_blocks, int n, const int16_t *samples, size_t sample_pitch, int blocks, uint8_t *slots,
                             size_t slot_pitch, size_t slot_bytes, int32_t *sizes, int16_t *recon, size_t recon_pitch, void *stats, int threads);
extern "C" uint64_t aenc_host_frame_bytes(int codec, int C, int blocks);
extern "C" int mux_host_run_audio(int container, uint32_t width, uint32_t height, uint32_t fps_rate, uint32_t fps_scale, uint32_t fps_raw, int max_keys, int n,
                                  int T, uint8_t *files, size_t pitch, size_t capacity, const uint8_t *slots, size_t slot_pitch, size_t slot_bytes,
                                  const int32_t *sizes, const uint8_t *key_flags, int64_t *bytes_out, int32_t *status_out, int audio_codec,
                                  uint32_t audio_frequency, int audio_channels, const uint8_t *stream_idx);
extern "C" uint64_t mux_host_framed_bytes_audio(int container, uint64_t stream_bytes);
extern "C" uint64_t mux_host_fixed_bytes_audio(int container, int key_frames, int audio);

int main(int argc, char **argv) {
  if (argc != 7) return 2;
  const int codec = atoi(argv[1]), n = atoi(argv[2]), C = atoi(argv[3]), B = atoi(argv[4]);
  if (n < 1 || C < 1 || C > 8 || B < 1) return 2;
  const size_t S = (size_t)256 * B, frame = (size_t)aenc_host_frame_bytes(codec, C, B);
  if (!frame) return 3;
  // exact-size heap buffers: one sample, one byte outside is the sanitizer's to report (pitches equal the lengths)
  std::vector<int16_t> x((size_t)n * C * S), recon(x.size());
  std::vector<uint8_t> slots((size_t)n * frame), stats((size_t)n * C * 16);
  std::vector<int32_t> sizes(n);
  FILE *f = fopen(argv[5], "rb");
  if (!f || fread(x.data(), 2, x.size(), f) != x.size()) return 2;
  fclose(f);
  if (aenc_host_run(codec, n, C, B, n, x.data(), S, B, slots.data(), frame, frame, sizes.data(), recon.data(), S, stats.data(), 2) != 0) return 3;
  // one clip, n appends, each an audio frame
  const size_t capacity = (size_t)mux_host_fixed_bytes_audio(0, 0, 1) + (size_t)n * (size_t)mux_host_framed_bytes_audio(0, frame);
  std::vector<uint8_t> file(capacity, 0xA5), keys(n, 0), idx(n, 1);
  int64_t bytes = 0;
  int32_t status = -1;
  if (mux_host_run_audio(0, 48, 32, 30, 1, 0, 0, 1, n, file.data(), capacity, capacity, slots.data(), frame, frame, sizes.data(), keys.data(), &bytes, &status, codec,
                         32000, C, idx.data()) != 0 ||
      status != 0 || (size_t)bytes != capacity)
    return 3;
  f = fopen(argv[6], "wb");
  if (!f || fwrite(slots.data(), 1, slots.size(), f) != slots.size() || fwrite(recon.data(), 2, recon.size(), f) != recon.size() ||
      fwrite(stats.data(), 1, stats.size(), f) != stats.size() || fwrite(file.data(), 1, file.size(), f) != file.size())
    return 2;
  fclose(f);
  return 0;
}
