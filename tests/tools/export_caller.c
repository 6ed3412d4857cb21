/* export_caller.c -- a plain C caller of the export entry points (mobi_host_alloc, mobi_batch_export, mobi_batch_export_wait / _query):
 * nothing but include/mobiclip_hip.h and libc.
 *
 *   export_caller <stream.bin> <width> <height> <version> <n_frames> <off_0> ... <off_n> <out.bin>
 *
 * Decodes the stream as clip 1 of a batch of two (clip 0 gets the same frames), and after every frame exports clip 1's picture as I420
 * into mobi_host_alloc memory, waits for the ticket and appends the bytes to out.bin; then exports the last min(6, n_frames) frames of
 * both clips in ONE call and appends those too (frame-major, clip 0 then clip 1).  Prints the rc of every frame.
 * tests/test_export_c_caller.py builds it with gcc and hashes what it wrote against tests/golden/golden.json.  Test tool only. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mobiclip_hip.h"

static int test_device(void) { const char *e = getenv("MOBI_DEVICE"); return e ? atoi(e) : 0; }

int main(int argc, char **argv) {
  if (argc < 7) { fprintf(stderr, "usage: see export_caller.c\n"); return 2; }
  const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]);
  const int version = atoi(argv[4]), nf = atoi(argv[5]);
  if (argc != 7 + nf + 1) { fprintf(stderr, "expected %d frame offsets and an output path\n", nf + 1); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *data = (uint8_t *)malloc((size_t)len);
  if (!data || fread(data, 1, (size_t)len, f) != (size_t)len) { fprintf(stderr, "read failed\n"); return 2; }
  fclose(f);
  FILE *out = fopen(argv[6 + nf + 1], "wb");
  if (!out) { perror(argv[6 + nf + 1]); return 2; }
  mobi_batch *b = mobi_batch_create(2, w, h, version, test_device());
  if (!b) { fprintf(stderr, "mobi_batch_create: %s\n", mobi_error_string(MOBI_E_DEVICE)); return 3; }
  const size_t pic = (size_t)w * h * 3 / 2;
  uint8_t *dst = (uint8_t *)mobi_host_alloc(pic * 12);
  if (!dst) { fprintf(stderr, "mobi_host_alloc failed\n"); return 3; }
  uint64_t t = 0;
  if (mobi_batch_export(b, MOBI_EXPORT_I420, 0, 1, 0, 1, dst, pic, &t) != MOBI_E_NULLREF) { fprintf(stderr, "export before the first frame\n"); return 4; }
  for (int i = 0; i < nf; i++) {
    const int32_t o = atoi(argv[6 + i]);
    const int32_t e = atoi(argv[6 + i + 1]);
    const uint8_t *d[2] = {data, data};
    size_t l[2] = {(size_t)e, (size_t)e};
    int32_t offs[2] = {o, o};
    int rc[2] = {0, 0};
    int r = mobi_batch_decode(b, d, l, offs, rc);
    if (r != MOBI_OK) { fprintf(stderr, "mobi_batch_decode: %s\n", mobi_error_string(r)); return 5; }
    printf("%d %d %d\n", i, rc[1], offs[1]);
    r = mobi_batch_export(b, MOBI_EXPORT_I420, 0, 1, 1, 1, dst, pic * 12, &t);
    if (r != MOBI_OK) { fprintf(stderr, "mobi_batch_export: %s\n", mobi_error_string(r)); return 6; }
    if (mobi_batch_export_wait(b, t) != MOBI_OK || mobi_batch_export_query(b, t) != 1) { fprintf(stderr, "export wait\n"); return 7; }
    fwrite(dst, 1, pic, out);
  }
  const int k = nf < 6 ? nf : 6;
  int r = mobi_batch_export(b, MOBI_EXPORT_I420, k - 1, k, 0, 2, dst, pic * 12, &t);
  if (r != MOBI_OK || mobi_batch_export_wait(b, t) != MOBI_OK) { fprintf(stderr, "mobi_batch_export (all): %s\n", mobi_error_string(r)); return 8; }
  fwrite(dst, 1, pic * 2 * (size_t)k, out);
  fclose(out);
  mobi_batch_destroy(b);
  mobi_host_free(dst);
  free(data);
  return 0;
}
