// learn_driver — the record-shape template learner (csrc/tfrg_learn.cpp) on its own, for the
// sanitizer run of tests/test_learn_sanitized.py (host code only: no device, nothing loaded into
// Python).  usage: learn_driver FILE.tfrecord KEYHEX:KIND [KEYHEX:KIND ...]   (kind 1 bytes, 2 float,
// 3 int64; one slot per argument). Prints the template count, the window words W and the
// window-form template words in hex.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/tfrg.h"
#include "../tfrecords-reader_amd/csrc/tfrg_layout.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s FILE KEYHEX:KIND ...\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  // (an exact-size heap copy: a read past the file's end is a read past the allocation)
  const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  // the schema: distinct keys in order of first appearance, one slot per argument
  std::vector<std::string> keys;
  std::vector<uint32_t> slot_key;
  std::vector<uint8_t> slot_kind;
  for (int i = 2; i < argc; ++i) {
    const char* colon = strchr(argv[i], ':');
    if (!colon || (colon - argv[i]) % 2) return 2;
    std::string key;
    for (const char* p = argv[i]; p < colon; p += 2) key.push_back((char)strtoul(std::string(p, 2).c_str(), nullptr, 16));
    auto it = std::find(keys.begin(), keys.end(), key);
    if (it == keys.end()) it = keys.insert(keys.end(), key);
    slot_key.push_back((uint32_t)(it - keys.begin()));
    slot_kind.push_back((uint8_t)atoi(colon + 1));
  }
  std::vector<uint8_t> blob;
  std::vector<uint64_t> key_off{0};
  for (const std::string& k : keys) {
    blob.insert(blob.end(), k.begin(), k.end());
    key_off.push_back(blob.size());
  }
  // the frames as their length fields give them: u64 length, u32 CRC, payload, u32 CRC. A frame
  // that runs past the file is kept as given (the learner must refuse it) and ends the index.
  std::vector<uint64_t> start, end;
  for (uint64_t pos = 0; pos + 12 <= file.size();) {
    uint64_t len;
    memcpy(&len, file.data() + pos, 8);
    const uint64_t e = pos + 16 + len;  // (may wrap: kept as it comes out)
    start.push_back(pos);
    end.push_back(e);
    if (e > file.size() || e <= pos) break;
    pos = e;
  }
  std::vector<uint32_t> words((size_t)TFRG_TPL_MAX * tfrg::kLtWords, 0u);
  uint32_t W = 0;
  const int nt = tfrg_learn_templates_host((uint32_t)keys.size(), blob.data(), key_off.data(), nullptr,
                                           (uint32_t)slot_key.size(), slot_key.data(), slot_kind.data(), file.data(),
                                           file.size(), start.data(), end.data(), (uint32_t)start.size(), 0, words.data(),
                                           words.size(), &W);
  if (nt < 0) {
    fprintf(stderr, "tfrg_learn_templates_host: %d\n", nt);
    return 1;
  }
  printf("templates %d\nW %u\nwords", nt, W);
  for (size_t i = 0; i < (size_t)nt * tfrg::kLtWords; ++i) printf(" %x", words[i]);
  printf("\n");
  return 0;
}
