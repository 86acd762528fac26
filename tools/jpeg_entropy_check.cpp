// Stand-alone check of the host JPEG entropy decoder (mega/pytorch_amd/csrc/jpeg_entropy.h) for sanitizer builds:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_entropy_check.cpp -o check
//   ./check good.jpg stream1 stream2 ...
// The first file must decode; every other file (truncated, corrupted, refused streams) is probed and, if the probe accepts
// it, decoded twice: against its own info and against the first file's.  Input and output live in heap blocks of exactly
// their size, so a read or write one byte outside either is a sanitizer report.  Whatever the decoder answers is fine; the
// program exits 0 unless the first file fails, a file cannot be read, or an accepted decode left an element unwritten.
// No GPU library is involved: this includes the header alone.
#include <stdio.h>
#include <stdlib.h>

#include "../mega/pytorch_amd/csrc/jpeg_entropy.h"

static unsigned char* read_file(const char* path, long long* n) {
  FILE* f = fopen(path, "rb");
  if (!f) return nullptr;
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* d = (unsigned char*)malloc(sz > 0 ? (size_t)sz : 1);
  if (sz > 0 && fread(d, 1, (size_t)sz, f) != (size_t)sz) {
    free(d);
    d = nullptr;
  }
  fclose(f);
  *n = sz;
  return d;
}

// decode into an exact-size block pre-filled with a sentinel no coefficient of these small images takes; 0 / 1 / 2 as the
// decoder says, -1 if it said OK and a sentinel survived
static int decode_checked(const unsigned char* d, long long n, const int* info) {
  const long long elems = info[11];
  int16_t* out = (int16_t*)malloc((size_t)elems * sizeof(int16_t));
  for (long long i = 0; i < elems; ++i) out[i] = (int16_t)0x7A7A;
  int rc = mega_jpeg::entropy_decode(d, n, info, out, elems);
  if (rc == mega_jpeg::JPG_OK) {
    for (long long i = 0; i < elems; ++i)
      if (out[i] == (int16_t)0x7A7A) rc = -1;
  }
  free(out);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s good.jpg [stream ...]\n", argv[0]);
    return 2;
  }
  int first[mega_jpeg::INFO_INTS];
  int counts[3] = {0, 0, 0};
  for (int a = 1; a < argc; ++a) {
    long long n = 0;
    unsigned char* d = read_file(argv[a], &n);
    if (!d) {
      fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    int info[mega_jpeg::INFO_INTS];
    int rc = mega_jpeg::probe(d, n, info);
    if (rc == mega_jpeg::JPG_OK) {
      if (a == 1) memcpy(first, info, sizeof(first));
      rc = decode_checked(d, n, info);
      const int rc2 = decode_checked(d, n, first);
      if (rc < 0 || rc2 < 0) {
        fprintf(stderr, "%s: decoded without writing every element\n", argv[a]);
        return 1;
      }
    }
    if (a == 1 && rc != mega_jpeg::JPG_OK) {
      fprintf(stderr, "%s: the reference stream does not decode (%d)\n", argv[a], rc);
      return 1;
    }
    ++counts[rc];
    free(d);
  }
  printf("%d streams: %d decoded, %d refused, %d corrupt\n", argc - 1, counts[0], counts[1], counts[2]);
  return 0;
}
