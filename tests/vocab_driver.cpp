// vocab_driver.cpp — a stand-alone program over the host half of the vocabulary object (tfrg_hash64,
// tfrg_vocab_create with device -1, tfrg_vocab_info, tfrg_vocab_lookup_host, tfrg_vocab_destroy in
// csrc/tfrg_host.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_vocab_sanitized.py. Usage: vocab_driver WORDS QUERIES. Both files hold byte strings as a u32
// little-endian length followed by the bytes. Prints the create status, the table's figures, every
// word's and every query's hash and looked-up id; then the refusals' statuses.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/tfrg.h"

static bool read_strings(const char* path, std::vector<std::string>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint32_t n;
  while (fread(&n, 4, 1, f) == 1) {
    std::string s(n, '\0');
    if (n && fread(&s[0], 1, n, f) != n) {
      fclose(f);
      return false;
    }
    out->push_back(s);
  }
  fclose(f);
  return true;
}

// the strings packed into a heap blob of exactly their size (so a read past a word is a finding)
static tfrg_vocab* create(const std::vector<std::string>& words, const int64_t* ids, int* rc) {
  std::vector<uint8_t> blob;
  std::vector<uint64_t> offs(1, 0);
  for (const std::string& w : words) {
    blob.insert(blob.end(), w.begin(), w.end());
    offs.push_back(blob.size());
  }
  tfrg_vocab* v = nullptr;
  *rc = tfrg_vocab_create(-1, blob.data(), offs.data(), words.size(), ids, &v);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<std::string> words, queries;
  if (!read_strings(argv[1], &words) || !read_strings(argv[2], &queries)) return 2;
  std::vector<int64_t> ids(words.size());
  for (size_t i = 0; i < ids.size(); ++i) ids[i] = 1000 - 3 * (int64_t)i;
  for (int with_ids = 0; with_ids < 2; ++with_ids) {
    int rc;
    tfrg_vocab* v = create(words, with_ids ? ids.data() : nullptr, &rc);
    printf("create %d\n", rc);
    if (!v) continue;
    uint64_t n = 0, cap = 0, dev = 0;
    uint32_t probe = 0;
    if (tfrg_vocab_info(v, &n, &cap, &probe, &dev) != 0) return 3;
    printf("info %llu %llu %u %llu\n", (unsigned long long)n, (unsigned long long)cap, probe, (unsigned long long)dev);
    for (const std::vector<std::string>* list : {&words, &queries})
      for (const std::string& s : *list) {
        // (an exact-size heap copy: the lookup may not read past the query either)
        std::vector<uint8_t> q(s.begin(), s.end());
        printf("%016llx %lld\n", (unsigned long long)tfrg_hash64(q.data(), q.size()),
               (long long)tfrg_vocab_lookup_host(v, q.data(), q.size(), -7));
      }
    if (tfrg_vocab_destroy(v) != 0) return 3;
  }
  // refusals: a duplicate of the last word, descending offsets, too many words; then the empty vocabulary
  int rc;
  if (!words.empty()) {
    std::vector<std::string> dup = words;
    dup.push_back(words.back());
    tfrg_vocab* v = create(dup, nullptr, &rc);
    printf("duplicate %d %d\n", rc, v != nullptr);
  }
  const uint8_t two[4] = {'a', 'b', 'c', 'd'};
  const uint64_t down[3] = {0, 3, 2};
  tfrg_vocab* v = nullptr;
  rc = tfrg_vocab_create(-1, two, down, 2, nullptr, &v);
  printf("descending %d %d\n", rc, v != nullptr);
  rc = tfrg_vocab_create(-1, two, down, 1ull << 31, nullptr, &v);
  printf("too_many %d %d\n", rc, v != nullptr);
  rc = tfrg_vocab_create(-1, nullptr, nullptr, 0, nullptr, &v);
  printf("empty %d %lld\n", rc, (long long)tfrg_vocab_lookup_host(v, two, 0, -7));
  if (tfrg_vocab_destroy(v) != 0) return 3;
  return 0;
}
