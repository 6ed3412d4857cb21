/* sink_caller.c -- the clip sink driven from plain C (tests/test_sink_gpu.py): include/mobiclip_hip.h, libc and three calls of the HIP
 * runtime for the tensor's device memory (declared here: a C caller has no HIP headers).
 *   sink_caller stream.bin W H version n_clips n_frames off[0] .. off[n_frames] T stride
 * Every clip decodes the same stream, as ONE group of n_frames frames, finished by mobi_batch_gop_finish_all with a sink armed: planar
 * uint8, the whole picture at 16 x 12, (N, T, 3, 12, 16) contiguous, start[c] = c % 2.  Prints "fnv <checksum of the tensor> pending <n>
 * launches <n>"; exit status 0 when every call did what it should. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mobiclip_hip.h"

int hipMalloc(void **p, size_t bytes);
int hipFree(void *p);
int hipMemcpy(void *dst, const void *src, size_t bytes, int kind); /* kind 2: device to host */
int hipMemset(void *dst, int value, size_t bytes);

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } \
  } while (0)

int main(int argc, char **argv) {
  CHECK(argc >= 9);
  const int W = atoi(argv[2]), H = atoi(argv[3]), version = atoi(argv[4]), n = atoi(argv[5]), nf = atoi(argv[6]);
  CHECK(n >= 1 && n <= 64 && nf >= 1 && nf <= 64 && argc == 7 + nf + 1 + 2);
  size_t off[65];
  for (int f = 0; f <= nf; f++) off[f] = (size_t)atol(argv[7 + f]);
  const int T = atoi(argv[8 + nf]), stride = atoi(argv[9 + nf]);
  FILE *fp = fopen(argv[1], "rb");
  CHECK(fp);
  uint8_t *data = malloc(off[nf]);
  CHECK(data && fread(data, 1, off[nf], fp) == off[nf]);
  fclose(fp);

  mobi_batch *b = mobi_batch_create(n, (uint32_t)W, (uint32_t)H, version, 0);
  CHECK(b);
  CHECK(mobi_batch_set_parse_mode(b, 1) == MOBI_OK);
  const int ow = 16, oh = 12;
  const size_t elems = (size_t)n * T * 3 * oh * ow;
  void *dst = NULL;
  CHECK(hipMalloc(&dst, elems) == 0 && hipMemset(dst, 0xA5, elems) == 0);
  int32_t start[64];
  for (int c = 0; c < n; c++) start[c] = c % 2;
  mobi_sink s;
  memset(&s, 0, sizeof(s));
  s.format = MOBI_EXPORT_RGB_PLANAR; s.dtype = MOBI_DTYPE_U8;
  s.out_w = ow; s.out_h = oh; s.n_frames = T; s.stride = stride; s.start = start;
  s.chan_stride = oh * ow; s.frame_stride = 3 * s.chan_stride; s.clip_stride = T * s.frame_stride;
  s.dst = dst; s.dst_bytes = elems;
  CHECK(mobi_sink_check(&s, n, (uint32_t)W, (uint32_t)H) == MOBI_OK);
  s.dst_bytes = elems - 1;
  CHECK(mobi_batch_set_sink(b, &s) == MOBI_E_ARG && mobi_batch_sink_pending(b) == 0);
  s.dst_bytes = elems;
  CHECK(mobi_batch_set_sink(b, &s) == MOBI_OK && mobi_batch_sink_pending(b) == n * T);

  const size_t nv = (size_t)n * nf;
  const uint8_t **ptr = malloc(nv * sizeof(*ptr));
  size_t *len = malloc(nv * sizeof(*len));
  int32_t *offs = malloc(nv * sizeof(*offs)), *offs_out = malloc(nv * sizeof(*offs_out));
  int *rc = malloc(nv * sizeof(*rc));
  CHECK(ptr && len && offs && offs_out && rc);
  for (int f = 0; f < nf; f++)
    for (int c = 0; c < n; c++) { ptr[f * n + c] = data; len[f * n + c] = off[f + 1]; offs[f * n + c] = (int32_t)off[f]; }
  CHECK(mobi_batch_gop_begin(b, nf, ptr, len, offs) == MOBI_OK);
  CHECK(mobi_batch_set_sink(b, NULL) == MOBI_E_ARG); /* a group is begun */
  CHECK(mobi_batch_gop_frames_pending(b) == nf);
  CHECK(mobi_batch_gop_finish_all(b, offs_out, rc) == MOBI_OK);
  CHECK(mobi_batch_gop_frames_pending(b) == 0 && mobi_batch_gop_in_flight(b) == 0);
  for (size_t v = 0; v < nv; v++) CHECK(rc[v] == MOBI_OK && offs_out[v] > offs[v]);

  uint8_t *host = malloc(elems);
  CHECK(host && hipMemcpy(host, dst, elems, 2) == 0);
  uint64_t h = 1469598103934665603ull; /* FNV-1a, 64 bits */
  for (size_t i = 0; i < elems; i++) { h ^= host[i]; h *= 1099511628211ull; }
  printf("fnv %llu pending %d launches %ld\n", (unsigned long long)h, mobi_batch_sink_pending(b), mobi_batch_sink_launches(b));
  CHECK(mobi_batch_set_sink(b, NULL) == MOBI_OK);
  mobi_batch_destroy(b);
  CHECK(hipFree(dst) == 0);
  return 0;
}
