// implicit_off_driver — learn_shapes (csrc/tfrg_learn.cpp) on its own, for tests/test_implicit_off_host.py:
// the per-slot end-relative rule of Learned (off_rel, rel_off) beside len_const / const_len, which the
// C ABI reports only through a device context. Host code only: no device, nothing loaded into Python.
// usage: implicit_off_driver FILE.tfrecord KEYHEX:KIND [KEYHEX:KIND ...]   (kind 1 bytes, 2 float,
// 3 int64; one slot per argument; the file's frames are well formed). Prints one line each:
// templates, off_rel (hex), rel_off per slot, len_const, const_len per slot.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <unordered_map>
#include <vector>

#include "../tfrecords-reader_amd/csrc/tfrg_learn.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s FILE KEYHEX:KIND ...\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::unordered_map<std::string, uint32_t> key_id;
  std::vector<int32_t> key_slot;
  std::vector<uint8_t> slot_kind;
  for (int i = 2; i < argc; ++i) {
    const char* colon = strchr(argv[i], ':');
    if (!colon || (colon - argv[i]) % 2) return 2;
    std::string key;
    for (const char* p = argv[i]; p < colon; p += 2) key.push_back((char)strtoul(std::string(p, 2).c_str(), nullptr, 16));
    const int kind = atoi(colon + 1);
    if (kind < 1 || kind > 3) return 2;
    auto it = key_id.find(key);
    if (it == key_id.end()) {
      it = key_id.emplace(key, (uint32_t)key_id.size()).first;
      key_slot.insert(key_slot.end(), {0, -1, -1, -1});
    }
    key_slot[4ull * it->second + kind] = (int32_t)slot_kind.size();
    slot_kind.push_back((uint8_t)kind);
  }
  std::vector<uint64_t> start, end;
  for (uint64_t pos = 0; pos + 16 <= file.size();) {
    uint64_t len;
    memcpy(&len, file.data() + pos, 8);
    if (len > file.size() - pos - 16) break;
    start.push_back(pos);
    end.push_back(pos + 16 + len);
    pos += 16 + len;
  }
  const tfrg::TplSchema sch{key_id, key_slot, slot_kind};
  tfrg::Learned L;
  const uint32_t S = (uint32_t)slot_kind.size();
  const uint32_t nt = tfrg::learn_shapes(&sch, S, file.data(), file.size(), start.data(), end.data(),
                                         (uint32_t)start.size(), 0, L);
  printf("templates %u\noff_rel %llx\nrel_off", nt, (unsigned long long)(nt ? L.off_rel : 0ull));
  for (uint32_t k = 0; k < S; ++k) printf(" %d", nt && k < L.rel_off.size() ? L.rel_off[k] : 0);
  printf("\nlen_const %d\nconst_len", nt && L.len_const ? 1 : 0);
  for (uint32_t k = 0; k < S; ++k) printf(" %u", nt && k < L.const_len.size() ? L.const_len[k] : 0u);
  printf("\n");
  return 0;
}
