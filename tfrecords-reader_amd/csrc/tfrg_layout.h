// tfrg_layout.h — layout constants of the record-shape templates (window form), of their lane image
// and of the count word, shared by the host learner (tfrg_learn.cpp, plain C++) and the kernels. No
// HIP include: tfrg_internal.h includes this header, so every file sees the one definition.
#pragma once
#include <stdint.h>

namespace tfrg {

// Record-shape template: the payload of a canonical record whose every byte except list contents is
// fixed (keys, tags, lengths, entry order; for packed int64 lists the continuation bits, i.e. the
// varint boundaries). A record equal to it under the mask has exactly the template's dict (slots,
// ranks, counts, list locations), which k_tpl_lane (tfrg_tpl.hip) writes without a walk. Learned on
// the host (tfrg_learn_templates) and stored in WINDOW form: the last 4 W bytes of the framed record,
// [end - 4 W, end), as W little-endian words, so that the length field, its masked CRC, the payload
// and the stored data CRC (word W - 1) sit at template-constant positions for every record of the
// shape. Per window word: Bm = fixed bytes & mask, Mm = mask (0 outside the record, for the data
// CRC and for variable payload bits), Cm = the variable payload bits (the CRC's input). Payload
// byte p of a length-L record is window byte y = p + 4 W - 4 - L, at distance d = 4 W - 5 - y from
// the payload end; d < 32 for words W - 9 .. W - 2.
// Layout (u32): [kLtL] L, [kLtNe] entries, [kLtCrcw] bit j: word W - 9 + j has variable payload
// bits, [kLtChain] first word < W - 9 with variable payload bits (W: none), [kLtK] CRC-32C of the
// payload with every variable bit 0, [kLtAbsent] slots (< kLeanMaxSlots) absent from the shape,
// [kLtFrame] the frame class (below),
// [kLtEnt + 4 e] entries {slot | mode << 8 | spec << 12 | len << 16, rank, count word, pos}; mode 0:
// list location (pos = payload offset, len), 1: inline int64 varint of len bytes at window byte pos,
// 2: inline float at window byte pos, 3: inline bytes element of len bytes, pos = payload offset -
// 4 - L (the element's batch offset is end + pos); [kLtWin, +W) Bm, [+W, +2W) Mm, [+2W, +3W) Cm;
// [kLtSlot + 3 k] the same entries by SLOT k (< kLeanMaxSlots), so that k_tpl_lane stores slot k's
// columns once for the lanes of every template: {mode | len << 8 | rank << 16 (0: absent), pos,
// count word (0: absent)}.
// Frame class (kLtFrame; a shape is kept once per class its sample shows, tfrg_template_frames):
// 0 = spec, the length CRC a fixed template field and the data CRC computed, as above; 1 = unchecked,
// the frames of writers that leave both CRC fields 0 (the reference's test writers, crc=False):
// Bm 0 / Mm 0xff on the four length-CRC bytes and Bm 0 / Mm 0xffffffff on word W - 1, every other
// word as the spec template of the shape. A hit of an unchecked template proves both stored fields
// 0; its verdict is TFRG_V_LEN_MATCH, and k_tpl_lane takes the record only if its true masked
// payload CRC is not 0 as well (else the canonical walk's TFRG_V_DATA_CRC would be lost).
constexpr uint32_t kTplMaxL = 240, kTplMaxEntries = 16;  // (tfrg.h TFRG_TPL_MAX_PAYLOAD / _ENTRIES)
constexpr uint32_t kLtMaxW = 64;
constexpr uint32_t kLeanMaxSlots = 16;  // k_tpl_lane runs for schemas of at most this many slots
constexpr uint32_t kLtL = 0, kLtNe = 1, kLtCrcw = 2, kLtChain = 3, kLtK = 4, kLtAbsent = 5, kLtFrame = 6, kLtEnt = 8,
                   kLtWin = kLtEnt + 4 * kTplMaxEntries, kLtSlot = kLtWin + 3 * kLtMaxW,
                   kLtWords = kLtSlot + 3 * kLeanMaxSlots;

// Lane image of the templates (k_tpl_lane): each lane matches the template its record's payload
// length selects, so the template words are read per lane from LDS, where the workgroup copies this
// image. Built on the host from the window-form templates (tfrg_learn_templates) and stored after
// them in the template buffer (DevSchema::tpl_img). u32 words:
//   header [0, kLiHdr): [0] templates, [1] W, [2] words per template (kLiTw), [3] union over the
//     templates of kLtCrcw, [4] the smallest kLtChain, [5] the table words packed behind the image
//     (below), [6] / [7] a byte per table word j = 0 .. 3 / 4 .. 7: its place in the packed block;
//   [kLiSlotQ + k] slot k (< kLeanMaxSlots): qlo | qhi << 8 | kLiQValue (some template holds an
//     inline int64 / float there, in window words qlo .. qhi + 1) | kLiQSingle (no template has more
//     than one value there);
//   [kLiLut, + kLiLutWords) bytes: for payload length L <= kTplMaxL the first template of that
//     length (0xff: none);
//   [kLiTpl + t kLiTw(W)] template t: [0] L, [1] K, [2] the next template of the same length
//     (0xff: none; either frame class), [3] the frame class (kLtFrame), [4, 4 + W) Bm, [4 + W, 4 + 2 W) Mm, [4 + 2 W, 4 + 3 W) Cm, then per slot k 4 words
//     {mode | len << 8 | rank << 16 (0: absent), pos, count word (0: absent), 0}
//     ("Record-shape template" above for the fields).
// Packed position tables: the image (padded to whole 16 bytes) is followed by the CRC tables the
// templates look up and no others. Table word j < 8 is the four tables T_{28 - 4 j} .. T_{31 - 4 j}
// of window word W - 9 + j (256 entries each: kLiPtabWords u32); a word is packed when its
// bit of header word [3] is set, and word 7 (T_0 .. T_3) also when any template runs the chain.
// Every workgroup of k_tpl_lane copies the block into LDS: C1 packs 3 of the 8 words.
constexpr uint32_t kLiPtabWords = 4 * 256;
constexpr uint32_t kTplSample = 4096;  // host records the learner samples from a batch (TFRG_TPL_SAMPLE)
constexpr uint32_t kTplMaxLane = 32;  // templates kept for the lane kernel (the most frequent shapes; TFRG_TPL_MAX)
constexpr uint32_t kLiHdr = 8, kLiSlotQ = kLiHdr, kLiLut = kLiSlotQ + kLeanMaxSlots,
                   kLiLutWords = (kTplMaxL + 1 + 3) / 4, kLiTpl = (kLiLut + kLiLutWords + 3) & ~3u;
constexpr uint32_t kLiQValue = 1u << 16, kLiQSingle = 1u << 17;
constexpr uint32_t kLiTw(uint32_t W) { return 4 + 3 * W + 4 * kLeanMaxSlots; }
// LDS words the lane image may take: a workgroup's 64 KiB less k_tpl_lane's CRC tables when every
// table word is packed (32 KiB) and 512 B for its static words (tfrg_tpl.hip asserts it). With W = 64 this keeps 30
// templates, not kTplMaxLane (learn_shapes drops the least frequent ones).
constexpr uint32_t kLiMaxWords = (65536u - 32768u - 512u) / 4u;

// count column: bit 31 set = the slot's single value is stored inline in the loc word
constexpr uint32_t kCountInline = 0x80000000u;

}  // namespace tfrg
