// tfrg_learn.cpp — the record-shape template learner: sample records of a host batch -> window-form
// templates, their lane image, the packed CRC position tables and the speculative placement words
// (tfrg_layout.h, tfrg_learn.h). Plain host C++ with no device runtime: it parses record bytes from
// outside the program, so it is built and tested on its own as well (tests/learn_driver.cpp).
#include "tfrg_learn.h"

#include <string.h>

#include <algorithm>
#include <map>

#include "../../include/tfrg.h"
#include "crc32c.h"
#include "tfrg_layout.h"

namespace tfrg {

// include/tfrg.h documents these limits to callers
static_assert(TFRG_TPL_MAX == kTplMaxLane && TFRG_TPL_MAX_PAYLOAD == kTplMaxL && TFRG_TPL_MAX_ENTRIES == kTplMaxEntries &&
                  TFRG_TPL_MAX_SLOTS == kLeanMaxSlots && TFRG_TPL_SAMPLE == kTplSample,
              "tfrg.h mirrors tfrg_layout.h");

namespace {


// CRC-32C byte tables, built once (thread-safe: contexts of several host threads learn templates)
const CrcTables& crc_tables() {
  static const CrcTables T = [] {
    CrcTables t;
    crc_make_tables(&t);
    return t;
  }();
  return T;
}

// k_lane_count's hdr2 (tfrg_kernels.hip): 1-byte tag of wire type 2, 1..3-byte length, body in end
bool tpl_hdr2(const uint8_t* p, uint32_t L, uint32_t pos, uint32_t end, uint32_t& fn, uint32_t& off, uint32_t& len) {
  if (pos >= L || (p[pos] & 0x87u) != 0x02u) return false;
  fn = (p[pos] >> 3) & 0xfu;
  uint32_t q = pos + 1, l = 0;
  for (uint32_t nb = 0;; ++nb) {
    if (nb == 3 || q >= L) return false;
    const uint32_t b = p[q++];
    l |= (b & 0x7fu) << (7 * nb);
    if (!(b & 0x80u)) break;
  }
  off = q;
  len = l;
  return off <= end && l <= end - off;
}

struct Tpl {
  uint32_t L = 0;
  std::vector<uint8_t> bytes, mask;
  std::vector<uint32_t> ent;  // 4 words per entry
  uint32_t frame = 0;         // frame class (kLtFrame): 0 spec CRCs, 1 unchecked (both CRC fields 0)
  std::string key() const {  // identity: length, masked bytes, mask, frame class
    std::string k((const char*)&L, 4);
    for (uint32_t i = 0; i < L; ++i) k.push_back((char)(bytes[i] & mask[i]));
    k.append((const char*)mask.data(), mask.size());
    k.push_back((char)frame);
    return k;
  }
};

// The dict fast_walk (tfrg_kernels.hip) builds for this payload, as a template; false where
// fast_walk would bail (or the shape does not fit a template).
bool tpl_derive(const TplSchema* c, const uint8_t* p, uint32_t L, Tpl& t) {
  if (L < 2 || L > kTplMaxL) return false;
  t.L = L;
  t.bytes.assign(p, p + L);
  t.mask.assign(L, 0xffu);
  t.ent.clear();
  t.frame = 0;
  uint32_t fn, fo, fl;
  if (!tpl_hdr2(p, L, 0, L, fn, fo, fl) || fn != 1u || fo + fl != L) return false;
  std::vector<uint32_t> seen;
  uint32_t rank = 0;
  for (uint32_t q = fo; q < L;) {
    uint32_t en, eo, el, kn, ko, kl, vn, vo, vl, kind, lo, ll;
    if (!tpl_hdr2(p, L, q, L, en, eo, el) || en != 1u) return false;
    const uint32_t ee = eo + el;
    q = ee;
    if (!tpl_hdr2(p, L, eo, ee, kn, ko, kl) || kn != 1u) return false;
    if (!tpl_hdr2(p, L, ko + kl, ee, vn, vo, vl) || vn != 2u || vo + vl != ee) return false;
    if (!tpl_hdr2(p, L, vo, ee, kind, lo, ll) || lo + ll != ee || kind < 1u || kind > 3u) return false;
    if (kl > 256u) return false;
    const auto it = c->key_id.find(std::string((const char*)p + ko, kl));
    if (it == c->key_id.end()) return false;
    const uint32_t kid = it->second;
    if (c->key_slot[4ull * kid] & 1) return false;  // invalid UTF-8 key: the exact path
    const int32_t slot = c->key_slot[4ull * kid + kind];
    if (slot < 0 || std::find(seen.begin(), seen.end(), kid) != seen.end()) return false;
    seen.push_back(kid);
    uint32_t cnt = 0, nch = 0, c0o = 0, c0l = 0;
    const uint32_t le = lo + ll;
    for (uint32_t g = lo; g < le;) {
      uint32_t cf, co, cl;
      if (!tpl_hdr2(p, L, g, le, cf, co, cl) || cf != 1u) return false;
      g = co + cl;
      if (kind == TFRG_KIND_BYTES) {
        ++cnt;
        std::fill(t.mask.begin() + co, t.mask.begin() + co + cl, 0);
      } else if (kind == TFRG_KIND_FLOAT) {
        if (cl & 3u) return false;
        cnt += cl >> 2;
        std::fill(t.mask.begin() + co, t.mask.begin() + co + cl, 0);
      } else {  // packed varints: terminated, none longer than 10 bytes; their boundaries are fixed
        uint32_t run = 0;
        for (uint32_t i = co; i < co + cl; ++i) {
          t.mask[i] = 0x80u;
          if (p[i] & 0x80u) {
            if (++run >= 10u) return false;
          } else {
            run = 0;
            ++cnt;
          }
        }
        if (cl && (p[co + cl - 1] & 0x80u)) return false;
      }
      if (nch == 0) {
        c0o = co;
        c0l = cl;
      }
      ++nch;
    }
    if (rank >= 65534u || t.ent.size() / 4 >= kTplMaxEntries) return false;
    ++rank;
    uint32_t mode = 0, cw = cnt, a = lo, b = ll;
    if (cnt == 1u && nch == 1u) {
      if (kind == TFRG_KIND_BYTES) {
        mode = 3;
      } else if (kind == TFRG_KIND_FLOAT) {
        mode = 2;
      } else if (c0l <= 4u) {
        mode = 1;
      }
      if (mode) {
        cw = 1u | kCountInline;
        a = c0o;
        b = c0l;
      }
    }
    t.ent.insert(t.ent.end(), {(uint32_t)slot | (mode << 24), rank, cw, a | (b << 16)});
  }
  return !t.ent.empty();
}

// The speculative placement words (DevSchema::spec) of the slots that were a single inline value in
// all `all` sampled shapes / records (count[k] == all): ranks per kind in slot order up to the first
// slot of that kind that is not one. Returns whether any slot was placed.
bool place_single_slots(const TplSchema* c, uint32_t S, const std::vector<uint32_t>& count, uint32_t all,
                        std::vector<uint32_t>& spec) {
  bool any = false;
  uint32_t rank[4] = {0, 0, 0, 0};
  bool open[4] = {true, true, true, true};
  for (uint32_t k = 0; k < S; ++k) {
    const uint32_t kd = c->slot_kind[k] & 3u;
    if (!open[kd]) continue;
    if (count[k] == all) {
      spec[k] = ((++rank[kd]) << 2) | kd;
      any = true;
    } else {
      open[kd] = false;
    }
  }
  return any;
}

}  // namespace

uint32_t learn_shapes(const TplSchema* c, uint32_t S, const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_start,
                      const uint64_t* h_end, uint32_t n, uint32_t flags, Learned& out) {
  std::map<std::string, std::pair<uint32_t, Tpl>> seen;  // (shape, frame class) -> (records, template)
  Tpl t;
  // up to kTplSample (4,096) records spread over the whole batch (not its first ones: ids that grow with the
  // record index give the first records shapes the rest of a file does not have)
  const uint32_t lim = n < kTplSample ? n : kTplSample;
  for (uint32_t j = 0; j < lim; ++j) {
    const uint32_t i = (uint32_t)((uint64_t)j * n / lim);
    uint64_t a = h_start[i], e = h_end[i];
    if (e > nbytes || e < a) continue;
    bool unchecked = false;
    if (!(flags & TFRG_FLAG_PAYLOAD_ONLY)) {  // framed: a length field matching the range
      if (e - a < 16) continue;
      uint64_t len = 0;
      memcpy(&len, h_bytes + a, 8);
      if (len != e - a - 16) continue;
      // unchecked frame (the reference's writers): both CRC fields 0 where the spec length CRC is not
      uint32_t lc = 0, dc = 0;
      memcpy(&lc, h_bytes + a + 8, 4);
      memcpy(&dc, h_bytes + e - 4, 4);
      unchecked = lc == 0 && dc == 0 && tfrg_masked_crc32c(h_bytes + a, 8) != 0;
      a += 12;
      e -= 4;
    }
    if (!tpl_derive(c, h_bytes + a, (uint32_t)(e - a > 0xffffffffull ? 0 : e - a), t)) continue;
    t.frame = unchecked ? 1u : 0u;
    auto& slot = seen[t.key()];
    if (!slot.first) slot.second = t;
    ++slot.first;
  }
  std::vector<std::pair<uint32_t, const Tpl*>> order;
  // shapes seen at least twice in a large sample (a one-off shape would only cost the kernel a
  // template and could turn a speculatively placed slot irregular), the most frequent first
  const uint32_t min_count = lim >= 256u ? 2u : 1u;
  for (auto& kv : seen)
    if (kv.second.first >= min_count) order.push_back({kv.second.first, &kv.second.second});
  std::stable_sort(order.begin(), order.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
  uint32_t nt = (uint32_t)std::min<size_t>(order.size(), kTplMaxLane);
  if (!nt) return 0;
  // the window the longest kept shape needs, and as many templates as fit LDS beside the CRC tables
  // at that window (the least frequent dropped first; a smaller maximum length may shrink W again)
  auto window_of = [&](uint32_t m) {
    uint32_t mx = 0;
    for (uint32_t k = 0; k < m; ++k) mx = std::max(mx, order[k].second->L);
    return mx + 16 <= 64 ? 16u : (mx + 16 <= 128 ? 32u : 64u);
  };
  while (nt > 1 && kLiTpl + (uint64_t)nt * kLiTw(window_of(nt)) > kLiMaxWords) --nt;
  uint64_t kept = 0;
  for (uint32_t k = 0; k < nt; ++k) kept += order[k].first;
  out.full = kept == lim;
  // speculative placement (DevSchema::spec): slots that are an inline single value in every kept
  // template, taken per kind in slot order up to the first slot of that kind that is not one (its
  // column base n * rank then holds whenever every record is regular)
  std::vector<uint32_t> seen_inline(S, 0), spec(S ? S : 1, 0);
  for (uint32_t k = 0; k < nt; ++k) {
    const Tpl& x = *order[k].second;
    for (size_t e = 0; e < x.ent.size(); e += 4) {
      const uint32_t slot = x.ent[e] & 0xffffffu, mode = x.ent[e] >> 24;
      if (mode && slot < S) ++seen_inline[slot];
    }
  }
  const bool have_spec = place_single_slots(c, S, seen_inline, nt, spec);
  // window form (tfrg_layout.h): the last 4 W bytes of every kept shape's framed record
  const uint32_t W = window_of(nt);
  const CrcTables& CT = crc_tables();
  std::vector<uint32_t> w((size_t)nt * kLtWords, 0);
  for (uint32_t k = 0; k < nt; ++k) {
    const Tpl& x = *order[k].second;
    const uint32_t L = x.L;
    uint32_t* d = &w[(size_t)k * kLtWords];
    std::vector<uint8_t> Bm(4 * W, 0), Mm(4 * W, 0), Cm(4 * W, 0);
    const uint32_t off = 4 * W - (L + 16);  // window byte of the record start
    const uint64_t L64 = L;
    const uint32_t lcrc = tfrg_masked_crc32c(reinterpret_cast<const uint8_t*>(&L64), 8);
    for (int i = 0; i < 8; ++i) {
      Bm[off + i] = (uint8_t)(L64 >> (8 * i));
      Mm[off + i] = 0xffu;
    }
    for (int i = 0; i < 4; ++i) {  // (unchecked frame: both CRC fields are 0, the data CRC's word W - 1)
      Bm[off + 8 + i] = x.frame ? 0u : (uint8_t)(lcrc >> (8 * i));
      Mm[off + 8 + i] = 0xffu;
      if (x.frame) Mm[4 * W - 4 + i] = 0xffu;
    }
    std::vector<uint8_t> fixed(L);
    for (uint32_t p = 0; p < L; ++p) {
      fixed[p] = x.bytes[p] & x.mask[p];
      Bm[off + 12 + p] = fixed[p];
      Mm[off + 12 + p] = x.mask[p];
      Cm[off + 12 + p] = (uint8_t)~x.mask[p];
    }
    auto word = [&](const std::vector<uint8_t>& v, uint32_t i) {
      return (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) |
             ((uint32_t)v[4 * i + 3] << 24);
    };
    uint32_t crcw = 0, chain = W;
    for (uint32_t i = 0; i < W; ++i) {
      d[kLtWin + i] = word(Bm, i);
      d[kLtWin + W + i] = word(Mm, i);
      d[kLtWin + 2 * W + i] = word(Cm, i);
      if (!word(Cm, i)) continue;
      if (i + 9 < W) chain = std::min(chain, i);
      else crcw |= 1u << (i - (W - 9));
    }
    if (chain < W) crcw |= 1u;  // the chain's state joins word W - 9
    d[kLtL] = L;
    d[kLtNe] = (uint32_t)(x.ent.size() / 4);
    d[kLtCrcw] = crcw;
    d[kLtChain] = chain;
    d[kLtK] = ~crc_update_bytes(CT, 0xffffffffu, fixed.data(), L);  // CRC-32C with every variable bit 0
    d[kLtFrame] = x.frame;
    out.frames |= 1u << x.frame;
    uint32_t present = 0;
    for (size_t e = 0; e < x.ent.size(); e += 4) {
      const uint32_t slot = x.ent[e] & 0xffffffu, mode = x.ent[e] >> 24;
      const uint32_t a = x.ent[e + 3] & 0xffffu, b = x.ent[e + 3] >> 16;
      uint32_t pos = a;  // mode 0: list location
      if (mode == 1 || mode == 2) pos = off + 12 + a;                  // window byte of the value
      else if (mode == 3) pos = (uint32_t)((int64_t)a - 4 - (int64_t)L);  // element = end + pos
      const uint32_t sp = slot < S && spec[slot] ? 1u : 0u;
      uint32_t* q = d + kLtEnt + e;  // (e steps by 4 words)
      q[0] = (slot & 0xffu) | (mode << 8) | (sp << 12) | (b << 16);
      q[1] = x.ent[e + 1];
      q[2] = x.ent[e + 2];
      q[3] = pos;
      if (slot < 32) present |= 1u << slot;
      if (slot < kLeanMaxSlots) {  // the slot table (ranks < 2^16: tpl_derive caps them)
        uint32_t* z = d + kLtSlot + 3 * slot;
        z[0] = mode | (b << 8) | (x.ent[e + 1] << 16);
        z[1] = pos;
        z[2] = x.ent[e + 2];
      }
    }
    d[kLtAbsent] = ~present & (S >= kLeanMaxSlots ? 0xffffu : ((1u << S) - 1u));
  }
  // the lane image (tfrg_layout.h kLi*): per-lane template words, the length table, per-slot ranges
  const uint32_t tw = kLiTw(W);
  std::vector<uint32_t> img(kLiTpl + (size_t)nt * tw, 0);
  img[0] = nt;
  img[1] = W;
  img[2] = tw;
  img[4] = W;
  std::vector<uint8_t> lut(kTplMaxL + 1, 0xffu);
  for (uint32_t k = 0; k < nt; ++k) {
    const uint32_t* d = &w[(size_t)k * kLtWords];
    uint32_t* q = &img[kLiTpl + (size_t)k * tw];
    const uint32_t L = d[kLtL];
    q[0] = L;
    q[1] = d[kLtK];
    q[2] = 0xffu;
    q[3] = d[kLtFrame];
    for (uint32_t i = 0; i < 3 * W; ++i) q[4 + i] = d[kLtWin + (i / W) * W + i % W];
    for (uint32_t s2 = 0; s2 < kLeanMaxSlots; ++s2) {
      const uint32_t* z = d + kLtSlot + 3 * s2;
      uint32_t* y = q + 4 + 3 * W + 4 * s2;
      y[0] = z[0];
      y[1] = z[1];
      y[2] = z[2];
      const uint32_t mode = z[0] & 0xffu, rk = z[0] >> 16;
      uint32_t& sq = img[kLiSlotQ + s2];
      if (rk && (mode == 1u || mode == 2u)) {  // an inline value in window words [pos / 4, pos / 4 + 1]
        const uint32_t qw = z[1] >> 2;
        const uint32_t lo = (sq & kLiQValue) ? std::min(sq & 0xffu, qw) : qw;
        const uint32_t hi = (sq & kLiQValue) ? std::max((sq >> 8) & 0xffu, qw) : qw;
        sq = (sq & kLiQSingle) | kLiQValue | lo | (hi << 8);
      }
      if (k == 0) sq |= kLiQSingle;
      if ((z[2] & ~kCountInline) > 1u) sq &= ~kLiQSingle;
    }
    img[3] |= d[kLtCrcw];
    img[4] = std::min(img[4], d[kLtChain]);
    // the length chain: templates of one length in order of frequency
    if (lut[L] == 0xffu) {
      lut[L] = (uint8_t)k;
    } else {
      uint32_t p = lut[L];
      while (img[kLiTpl + (size_t)p * tw + 2] != 0xffu) p = img[kLiTpl + (size_t)p * tw + 2];
      img[kLiTpl + (size_t)p * tw + 2] = k;
    }
  }
  memcpy(&img[kLiLut], lut.data(), lut.size());
  // the packed position tables (tfrg_layout.h, image words 5 .. 7): of the 8 table words only
  // those some kept template looks up, in word order; the chain runs on word 7's tables T_0 .. T_3
  {
    const uint32_t used = (img[3] & 0xffu) | (img[4] < W ? 0x80u : 0u);
    uint32_t np = 0;
    for (uint32_t j = 0; j < 8; ++j) {
      if (!(used & (1u << j))) continue;
      img[6 + j / 4] |= np << (8 * (j % 4));
      out.ptab.resize((size_t)(np + 1) * kLiPtabWords);
      uint32_t* t = &out.ptab[(size_t)np * kLiPtabWords];
      for (uint32_t v = 0; v < 256; ++v) {  // T_d[v] = U(0, v followed by d zero bytes)
        uint32_t x = CT.t[0][v];
        for (uint32_t d = 0; d < 32; ++d) {
          if (d >= 28 - 4 * j && d < 32 - 4 * j) t[(d - (28 - 4 * j)) * 256 + v] = x;
          x = (x >> 8) ^ CT.t[0][x & 0xff];
        }
      }
      ++np;
    }
    img[5] = np;
  }
  // every slot present at the same key position (order word) in every kept shape: an optimistic
  // decode leaves the order column implicit (TFRG_IMPLICIT_ORDER)
  out.ord_const = S > 0 && S <= kLeanMaxSlots;
  for (uint32_t s2 = 0; out.ord_const && s2 < S; ++s2) {
    const uint32_t r0 = w[kLtSlot + 3 * s2] >> 16;
    out.ord_const = r0 != 0;
    for (uint32_t k = 1; out.ord_const && k < nt; ++k) out.ord_const = (w[(size_t)k * kLtWords + kLtSlot + 3 * s2] >> 16) == r0;
  }
  out.len_const = S > 0 && S <= kLeanMaxSlots;
  out.const_len.assign(S, 0u);
  for (uint32_t s2 = 0; out.len_const && s2 < S; ++s2) {
    if ((c->slot_kind[s2] & 3u) != TFRG_KIND_BYTES) continue;
    const uint32_t z0 = w[kLtSlot + 3 * s2];
    out.len_const = (z0 & 0xffu) == 3u && (z0 >> 16) != 0;
    for (uint32_t k = 1; out.len_const && k < nt; ++k) {
      const uint32_t zk = w[(size_t)k * kLtWords + kLtSlot + 3 * s2];
      out.len_const = (zk & 0xffu) == 3u && (zk >> 16) != 0 && ((zk >> 8) & 0xffu) == ((z0 >> 8) & 0xffu);
    }
    out.const_len[s2] = (z0 >> 8) & 0xffu;
  }
  // a bytes slot that is one inline element at one end-relative position in every kept shape
  out.off_rel = 0;
  out.rel_off.assign(S, 0);
  for (uint32_t s2 = 0; s2 < S && s2 < kLeanMaxSlots && s2 < 64u; ++s2) {
    if ((c->slot_kind[s2] & 3u) != TFRG_KIND_BYTES) continue;
    const uint32_t z0 = w[kLtSlot + 3 * s2], p0 = w[kLtSlot + 3 * s2 + 1];
    bool rel = (z0 & 0xffu) == 3u && (z0 >> 16) != 0;
    for (uint32_t k = 1; rel && k < nt; ++k) {
      const uint32_t* zk = &w[(size_t)k * kLtWords + kLtSlot + 3 * s2];
      rel = (zk[0] & 0xffu) == 3u && (zk[0] >> 16) != 0 && zk[1] == p0;
    }
    if (!rel) continue;
    out.off_rel |= 1ull << s2;
    out.rel_off[s2] = (int32_t)p0;
  }
  out.w = std::move(w);
  out.spec = std::move(spec);
  out.img = std::move(img);
  out.img.resize((out.img.size() + 3) & ~(size_t)3, 0u);  // (the tables after it: 16-byte aligned)
  out.W = W;
  out.have_spec = have_spec;
  return nt;
}

// Speculative placement without record shapes (records too large or too varied for a template,
// C2's flowers): a slot whose list is one inline value -- one bytes element, one float, one int64
// varint of <= 4 bytes (k_lane_count's inline rule) -- in every record of the sample that decodes,
// by the host decoder (the reference's semantics). Ranks per kind in slot order up to the first slot
// of that kind that is not one (as learn_shapes). Returns whether any slot was placed.
bool learn_single_slots(const TplSchema* c, uint32_t S, const uint8_t* h_bytes, uint64_t nbytes,
                        const uint64_t* h_start, const uint64_t* h_end, uint32_t n, uint32_t flags,
                        std::vector<uint32_t>& spec) {
  spec.assign(S ? S : 1, 0u);
  if (!S || !n) return false;
  tfrg_host_ctx* hc = nullptr;
  if (tfrg_host_ctx_create(&hc)) return false;
  std::vector<uint32_t> single(S, 0u);
  uint32_t m = 0;
  const uint32_t lim = n < kTplSample ? n : kTplSample;
  for (uint32_t j = 0; j < lim; ++j) {
    const uint32_t i = (uint32_t)((uint64_t)j * n / lim);
    uint64_t a = h_start[i], e = h_end[i];
    if (e > nbytes || e < a) continue;
    if (!(flags & TFRG_FLAG_PAYLOAD_ONLY)) {
      if (e - a < 16) continue;
      a += 12;
      e -= 4;
    }
    tfrg_host_record rec;
    if (tfrg_host_decode(hc, h_bytes + a, e - a, flags, &rec) || rec.status != TFRG_OK) continue;
    ++m;
    for (uint32_t k = 0; k < rec.n_entries; ++k) {
      const auto it = c->key_id.find(std::string((const char*)h_bytes + a + rec.key_off[k], rec.key_len[k]));
      if (it == c->key_id.end()) continue;
      const uint32_t kind = rec.kind[k];
      if (kind < 1 || kind > 3) continue;
      const int32_t slot = c->key_slot[4ull * it->second + kind];
      if (slot < 0 || (uint32_t)slot >= S || rec.val_cnt[k] != 1) continue;
      if (kind == TFRG_KIND_INT64) {
        const int64_t v = rec.i64[rec.val_off[k]];
        if (v < 0 || v >= (int64_t)1 << 28) continue;  // (more than 4 varint bytes: not inline)
      }
      ++single[slot];
    }
  }
  tfrg_host_ctx_destroy(hc);
  if (!m) return false;
  return place_single_slots(c, S, single, m, spec);
}

}  // namespace tfrg

using namespace tfrg;

extern "C" int tfrg_learn_templates_host(uint32_t n_keys, const uint8_t* key_blob, const uint64_t* key_offsets,
                                         const uint32_t* key_flags, uint32_t n_slots, const uint32_t* slot_key,
                                         const uint8_t* slot_kind, const uint8_t* h_bytes, uint64_t nbytes,
                                         const uint64_t* h_start, const uint64_t* h_end, uint32_t n, uint32_t flags,
                                         uint32_t* out, uint64_t cap, uint32_t* window_words) {
  if (n && (!h_bytes || !h_start || !h_end)) return TFRG_E_ARG;
  std::unordered_map<std::string, uint32_t> key_id;
  std::vector<int32_t> ks(4ull * (n_keys ? n_keys : 1), -1);
  for (uint32_t k = 0; k < n_keys; ++k) {
    key_id.emplace(std::string((const char*)key_blob + key_offsets[k], key_offsets[k + 1] - key_offsets[k]), k);
    ks[4ull * k] = (int32_t)(key_flags ? (key_flags[k] & 1u) : 0u);
  }
  for (uint32_t s2 = 0; s2 < n_slots; ++s2) {
    if (slot_key[s2] >= n_keys || slot_kind[s2] < 1 || slot_kind[s2] > 3) return TFRG_E_ARG;
    ks[4ull * slot_key[s2] + slot_kind[s2]] = (int32_t)s2;
  }
  std::vector<uint8_t> sk(slot_kind, slot_kind + n_slots);
  const TplSchema sch{key_id, ks, sk};
  Learned L;
  const uint32_t nt = learn_shapes(&sch, n_slots, h_bytes, nbytes, h_start, h_end, n, flags, L);
  if (window_words) *window_words = L.W;
  if (out && nt) memcpy(out, L.w.data(), std::min<uint64_t>(L.w.size(), cap) * 4);
  return (int)nt;
}
