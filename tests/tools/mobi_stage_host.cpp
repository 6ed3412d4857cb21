// mobi_stage_host.cpp -- TEST TOOL: the staged bitstream image of a device-parsed hand-over (csrc/mobi_handover.h: planner, header, gather,
// routing) behind a C entry point, so that tests/test_stage_image.py can hold it against a Python model of the layout without a GPU.
//
// With -DMOBI_STAGE_HOST_MAIN it is a stand-alone program for the host sanitizers: the test's two hand-overs (a step and a group of two frames
// of three clips of 2x2 macroblocks) with every frame and the image in a heap allocation of exactly its size, and checksums printed.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -DMOBI_STAGE_HOST_MAIN -I mobiclipdecoder_amd/csrc tests/tools/mobi_stage_host.cpp -o stage_host_san && ./stage_host_san
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mobi_handover.h"

// One hand-over.  group == 0: a step (on_host at once); else a group (the host parser's lanes keep their bytes, idle_from[n] rides), routed
// with on_host behind the gather when route != 0.  info[10]: hdr_bytes, bytes, max_len, reset_off, n_reset, idle_off, n_idle, idle_from_off,
// n_dev, n_iframes; boff / lens: [n * K].  The image goes to `image` when it fits image_cap.  Returns 0, or 1 when it did not fit.
extern "C" int mobi_stage_host_build(int n, int K, int n_mbs, const uint8_t *const *data, const size_t *len, const int32_t *offsets, const uint8_t *on_host,
                                     const uint8_t *idle_from, const int32_t *resets, int n_resets, int group, int route, uint8_t *image, size_t image_cap,
                                     uint64_t *info, uint64_t *boff, uint32_t *lens) {
  StageImage img;
  img.plan(n, K, n_mbs, data, len, offsets, group ? nullptr : on_host, idle_from, (size_t)n_resets, group != 0);
  const bool fits = img.bytes <= image_cap;
  if (fits) {
    img.write_header(image, resets, idle_from);
    for (size_t v = 0; v < img.lanes(); v++) img.gather(image, v, data, offsets);
    if (group && route) img.route(image, on_host);
  }
  const uint64_t out[10] = {img.hdr_bytes, img.bytes, img.max_len, img.reset_off, (uint64_t)img.n_reset, img.idle_off, (uint64_t)img.n_idle, img.idle_from_off,
                            (uint64_t)img.n_dev, (uint64_t)img.n_iframes};
  memcpy(info, out, sizeof out);
  memcpy(boff, img.boff.data(), img.lanes() * 8);
  memcpy(lens, img.lens.data(), img.lanes() * 4);
  return fits ? 0 : 1;
}

#ifdef MOBI_STAGE_HOST_MAIN
struct Lane { long size; int32_t offset; size_t len; int b0, b1; }; // size < 0: Data == null; b0, b1: the frame's first two bytes (-1: as generated)
static int run(const char *name, int K, const std::vector<Lane> &lanes, const uint8_t *on_host, const uint8_t *idle_from, const int32_t *resets, int group) {
  const int n = 3, n_mbs = 4;
  std::vector<uint8_t *> data;
  std::vector<size_t> len;
  std::vector<int32_t> off;
  uint32_t x = 5;
  for (const Lane &l : lanes) {
    uint8_t *p = l.size < 0 ? nullptr : new uint8_t[(size_t)l.size]; // its own allocation of exactly its size: a read past it is a heap overflow
    for (long i = 0; i < l.size; i++) p[i] = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
    if (l.b0 >= 0) p[l.offset] = (uint8_t)l.b0;
    if (l.b1 >= 0) p[l.offset + 1] = (uint8_t)l.b1;
    data.push_back(p); len.push_back(l.len); off.push_back(l.offset);
  }
  uint64_t info[10], boff[6];
  uint32_t lens[6];
  uint8_t none = 0;
  if (mobi_stage_host_build(n, K, n_mbs, data.data(), len.data(), off.data(), on_host, idle_from, resets, 2, group, 1, &none, 0, info, boff, lens) != 1) return 1; // sizes only
  uint8_t *image = new uint8_t[info[1]]; // exactly `bytes`
  memset(image, 0xAA, info[1]);
  if (mobi_stage_host_build(n, K, n_mbs, data.data(), len.data(), off.data(), on_host, idle_from, resets, 2, group, 1, image, info[1], info, boff, lens) != 0) return 1;
  uint64_t sum = 0;
  for (uint64_t i = 0; i < info[1]; i++) sum = sum * 31 + image[i];
  printf("%s: hdr %llu bytes %llu max_len %llu reset_off %llu idle_off %llu idle_from_off %llu n_dev %llu n_iframes %llu sum %016llx\n", name, (unsigned long long)info[0],
         (unsigned long long)info[1], (unsigned long long)info[2], (unsigned long long)info[3], (unsigned long long)info[5], (unsigned long long)info[7],
         (unsigned long long)info[8], (unsigned long long)info[9], (unsigned long long)sum);
  delete[] image;
  for (uint8_t *p : data) delete[] p;
  return 0;
}
int main() {
  const long big = 4 * 4096 + 64 + 100; // frame_bound + 100
  // (tests/test_stage_image.py has the same lanes and says what each is there for)
  const uint8_t step_host[3] = {0, 1, 0}, step_idle[3] = {1, 1, 0}, gop_host[3] = {0, 0, 1}, gop_idle[3] = {2, 1, 2};
  const int32_t step_resets[2] = {2, 0}, gop_resets[2] = {1, 2};
  int bad = run("step", 1, {{8, 3, 8, 0x12, 0x80}, {10, 11, 10, -1, -1}, {-1, -5, 0, -1, -1}}, step_host, step_idle, step_resets, 0);
  bad |= run("group", 2, {{1, 0, 1, 0xFF, -1}, {big + 7, 7, (size_t)big + 7, 0x55, 0x7F}, {4, -1, 4, -1, -1}, {-1, 0, 9, -1, -1}, {3, 0, 3, -1, -1}, {6, 6, 6, -1, -1}},
             gop_host, gop_idle, gop_resets, 1);
  return bad;
}
#endif
