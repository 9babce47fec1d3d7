// Stand-alone driver of the chunked framing index's CPU model (csrc/tfrg_frame_host.cpp) for
// tests/test_frame_index_sanitized.py: frame_index_driver <chunk> <file> indexes the file image,
// held in a heap buffer of exactly its size, and prints the summary and the rows.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../include/tfrg.h"

extern "C" int tfrg_index_chunked_host(const uint8_t* bytes, uint64_t nbytes, const uint64_t* piece_sizes,
                                       uint32_t n_pieces, uint32_t chunk, uint64_t* starts, uint64_t* ends,
                                       uint64_t cap, uint64_t* piece_records, tfrg_index_info* info);

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const uint32_t chunk = (uint32_t)strtoul(argv[1], nullptr, 10);
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* img = (uint8_t*)malloc(size ? (size_t)size : 1);  // (exact size: a read past the image is reported)
  if (size && fread(img, 1, (size_t)size, f) != (size_t)size) return 4;
  fclose(f);
  const uint64_t sz = (uint64_t)size, cap = sz + 1;
  std::vector<uint64_t> st(cap), en(cap);
  uint64_t pr = 0;
  tfrg_index_info info;
  const int rc = tfrg_index_chunked_host(img, sz, &sz, 1, chunk, st.data(), en.data(), cap, &pr, &info);
  if (rc) return 5;
  printf("info %llu %u %u %u %u %u %u piece %llu\n", (unsigned long long)info.n_records, info.fallback, info.tiled,
         info.first_start, info.n_chunks, info.repaired_chunks, info.repair_rounds, (unsigned long long)pr);
  if (!info.fallback)
    for (uint64_t i = 0; i < info.n_records && i < cap; ++i)
      printf("%llu %llu\n", (unsigned long long)st[i], (unsigned long long)en[i]);
  free(img);
  return 0;
}
