// tfrg_learn.h — the record-shape template learner (tfrg_learn.cpp): host code that parses sample
// records and builds the window-form templates, their lane image and the speculative placement
// words (tfrg_layout.h). It needs no device: tfrg_capi.cpp uploads a Learned into its context, and
// tfrg_learn_templates_host (include/tfrg.h) and tests/learn_driver.cpp run it on its own.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

namespace tfrg {

// the host key table the templates are derived against (tfrg_set_schema's, or a test's)
struct TplSchema {
  const std::unordered_map<std::string, uint32_t>& key_id;
  const std::vector<int32_t>& key_slot;  // [4 * key]: flags, slot per kind
  const std::vector<uint8_t>& slot_kind;
};

// Record shapes of a host sample -> window-form templates (tfrg_layout.h) + the speculative
// placement words.
struct Learned {
  std::vector<uint32_t> w, spec, img;  // window-form templates, spec words, lane image
  std::vector<uint32_t> ptab;          // the packed CRC position tables the image's header names
  uint32_t W = 0;
  bool have_spec = false;
  bool full = false;  // every sampled record took a kept template
  uint32_t frames = 0;  // frame classes of the kept templates: bit 0 spec, bit 1 unchecked
  bool ord_const = false;  // every slot (< kLeanMaxSlots) at one key position in every kept template
  // every bytes slot one element (mode 3) of one length in every kept template: an optimistic decode
  // leaves the bytes_len column implicit (TFRG_IMPLICIT_BYTES_LEN); const_len[k] that length
  bool len_const = false;
  std::vector<uint32_t> const_len;
  // bit k: bytes slot k (< 64) is one inline element (mode 3, present) at the same offset from the
  // record's end in every kept template; rel_off[k] that offset (the template's pos word, negative:
  // the element's batch offset is end + rel_off[k]). Per slot, whatever len_const says. An optimistic
  // decode with u32 offsets leaves such a slot's bytes_off words implicit (tfrg_info.implicit_off_slots)
  uint64_t off_rel = 0;
  std::vector<int32_t> rel_off;
};

// Returns the template count (0: none).
uint32_t learn_shapes(const TplSchema* c, uint32_t S, const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_start,
                      const uint64_t* h_end, uint32_t n, uint32_t flags, Learned& out);

// Speculative placement without record shapes. Returns whether any slot was placed.
bool learn_single_slots(const TplSchema* c, uint32_t S, const uint8_t* h_bytes, uint64_t nbytes,
                        const uint64_t* h_start, const uint64_t* h_end, uint32_t n, uint32_t flags,
                        std::vector<uint32_t>& spec);

}  // namespace tfrg
