// tfrg_vocab.h — tfrg_hash64 and the vocabulary object (include/tfrg.h: tfrg_vocab), as host C, the
// device (tfrg_ids.hip) and the C-ABI share them. No HIP header is needed: tfrg_host.cpp, which builds
// the table and looks words up on the host, is plain C++. The device half (upload, free) lives in
// tfrg_capi.cpp and reaches the host half through g_vocab_device.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIP__) || defined(__HIPCC__)
#define TFRG_HD __host__ __device__
#else
#define TFRG_HD
#endif

namespace tfrg {

// ------------------------------------------------------------------ tfrg_hash64
// h = seed; per 8-byte group w (little-endian, the last one zero-padded): h = (h ^ w) * mul; then the
// length and a 64-bit finalizer. One dependent 64-bit multiply per 8 bytes.
constexpr uint64_t kHashSeed = 0xcbf29ce484222325ull;
constexpr uint64_t kHashMul = 0x100000001b3ull;

TFRG_HD inline uint64_t hash_step(uint64_t h, uint64_t w) { return (h ^ w) * kHashMul; }

TFRG_HD inline uint64_t hash_finish(uint64_t h, uint64_t n) {
  h ^= n;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// (the host's: a little-endian host, as the rest of the library assumes)
inline uint64_t hash64(const uint8_t* p, uint64_t n) {
  uint64_t h = kHashSeed;
  uint64_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, p + i, 8);
    h = hash_step(h, w);
  }
  if (i < n) {
    uint64_t w = 0;
    memcpy(&w, p + i, (size_t)(n - i));
    h = hash_step(h, w);
  }
  return hash_finish(h, n);
}

constexpr uint32_t kVocabEmpty = 0xffffffffu;  // a table slot without a word

}  // namespace tfrg

// The object behind the public handle. The host arrays are always there; the device copies (one
// allocation: ids, table, offsets, blob) only for a vocabulary created with device >= 0.
struct tfrg_vocab {
  int device = -1;
  uint32_t max_probe = 0;  // the largest displacement of a word from its home slot
  uint32_t max_word = 0;   // the longest word's bytes
  std::vector<uint32_t> table;  // [capacity] word index, or kVocabEmpty
  std::vector<uint32_t> offs;   // [n_words + 1] word i is blob[offs[i] .. offs[i + 1])
  std::vector<uint8_t> blob;
  std::vector<int64_t> ids;     // [n_words]
  void* d_mem = nullptr;
  uint64_t device_bytes = 0;
  const int64_t* d_ids = nullptr;
  const uint32_t* d_table = nullptr;
  const uint32_t* d_offs = nullptr;
  const uint8_t* d_blob = nullptr;
  uint32_t d_blob_bound = 0;  // readable bytes of d_blob, a multiple of 4 (zeros after the blob)
};

namespace tfrg {
// The device half, registered by tfrg_capi.cpp where it is linked in (a program of the host files alone
// has none: tfrg_vocab_create then refuses device >= 0). Both return a TFRG_* code and set the error.
struct VocabDeviceOps {
  int (*upload)(tfrg_vocab* v);
  int (*release)(tfrg_vocab* v);  // synchronises the device, then frees
};
extern VocabDeviceOps g_vocab_device;
}  // namespace tfrg
