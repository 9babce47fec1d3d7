// tfrg_decode.cpp — launch_decode: the launch policy of one decode. Host code only; the kernels and
// their launchers (template arguments, LDS bytes, occupancy) live in the .hip files.
//
// Stages of one batch of records resident in HBM, in launch order:
//   k_tpl_lane    (tfrg_tpl.hip)    records that match a learned record-shape template: no walk, the
//                                   template's dict straight into the columns; the rest listed per
//                                   64-record group for k_lane_count.
//   k_lane_count  (tfrg_kernels.hip) one lane per record (all, or the listed groups): framing, CRC-32C
//                                   verdicts, the canonical walk; per-slot counts summed per tile.
//                                   Records it does not accept go to the slow list, accepted records
//                                   above lane_max to the streaming-CRC list.
//   k_body_count  (tfrg_kernels.hip) counts of the packed int64 bodies k_lane_count deferred.
//   k_tail_count  (tfrg_kernels.hip) the exact reference walk of the slow list; the streaming payload
//                                   CRC of the records above lane_max.
//   k_spine       (tfrg_scan.hip)    exclusive scan of the tile sums, column bases.
//   k_down_gather (tfrg_scan.hip)    row splits, inline single values.
//   k_tail_gather (tfrg_kernels.hip) out-of-line lists of lane records, records above lane_max.
//   (materialize: tfrg_bytes.hip, launched by the caller.)
// An optimistic decode ends after k_tpl_lane, or (without record shapes) after k_tail_count, whose
// last workgroup does the bookkeeping of the stages not launched; the host confirms it or re-runs
// the decode in full (tfrg_capi.cpp).
#include <algorithm>

#include "../../include/tfrg_status.h"
#include "tfrg_internal.h"

namespace tfrg {

const char* const kStageNames[kNumStages] = {"k_tpl_lane",    "k_lane_count",  "k_body_count", "k_tail_count", "k_spine",
                                             "k_down_gather", "k_tail_gather", "k_bytes"};

// k_tpl_lane's arguments: the column targets of every slot (as the kernels' spec_target: column rows
// n * (rank - 1) + r, r below the capacity)
static LeanArgs lean_args(const DevBatch& b, const DevSchema& sc, const DevOut& o, const LaunchCfg& cfg,
                          bool placing) {
  const bool nocrc = (b.flags & kFlagNoCrc) != 0;
  LeanArgs a{};
  a.n_tpl = sc.n_tpl;
  a.img_words = sc.tpl_img_words;
  a.tab_words = nocrc ? 0u : sc.tpl_tab_words;
  a.nocrc = nocrc ? 1u : 0u;
  a.strict = (b.flags & kFlagStrictCrc) ? 1u : 0u;
  a.uframes = cfg.tpl_unchecked ? 1u : 0u;
  a.cu_lds = cfg.tpl_cu_lds;
  a.stage_any = cfg.tpl_stage_any ? 1u : 0u;
  a.gpw_force = cfg.tpl_gpw;
  a.lane_max = cfg.lane_max;
  a.tsum = cfg.ran_optimistic ? nullptr : o.tsum;  // (placed slots: no scan; a re-run clears tsum)
  a.finish = cfg.ran_optimistic ? sc.slot_kind : nullptr;
  a.implicit = cfg.implicit;
  a.n_slots = sc.n_slots;
  a.tile_stride = o.tile_stride;
  const uint64_t n = b.n;
  for (uint32_t k = 0; k < sc.n_slots; ++k) {
    LeanTgt& t = a.tg[k];
    t.ord = o.order + k * n;
    t.cnt = o.count + k * n;
    t.loc = o.loc + k * n;
    t.rs = o.rs + k * (n + 1);
    const uint32_t sw = placing ? cfg.spec_h[k] : 0u;
    if (!sw) continue;
    const uint32_t kind = sw & 3u;
    const uint64_t base = n * ((sw >> 2) - 1u);
    const uint64_t cap = kind == TFRG_KIND_INT64 ? o.cap_i64 : kind == TFRG_KIND_FLOAT ? o.cap_f32 : o.cap_b;
    t.lim = cap > base ? (uint32_t)std::min<uint64_t>(cap - base, n) : 0u;
    t.kind = kind;
    if (kind == TFRG_KIND_INT64) t.v1 = o.i64 + base;
    else if (kind == TFRG_KIND_FLOAT) t.v1 = o.f32 + base;
    else t.v1 = o.b_off + base;
    t.v2 = o.b_len + base;
    t.no_off = kind == TFRG_KIND_BYTES && k < 64u && ((cfg.implicit_off >> k) & 1ull) ? 1u : 0u;
  }
  return a;
}

hipError_t launch_decode(const DevBatch& b, const DevSchema& sc, const DevOut& o, LaunchCfg& cfg,
                         const uint32_t* d_tab, const uint32_t* d_consts, hipStream_t st, hipEvent_t* ev) {
  auto mark = [&](int i) {
    if (ev) (void)hipEventRecord(ev[i], st);
  };
  auto mark_rest = [&](int from) {  // (an optimistic decode: the stages from here on are not launched)
    for (int i = from; i <= kStageMaterialize; ++i) mark(i);
    return hipGetLastError();
  };
  const uint32_t S = sc.n_slots, cus = (uint32_t)cfg.num_cus;
  const uint32_t n_tiles = (b.n + kTileRecs - 1) / kTileRecs;
  const bool fast_ok = schema_in_lds(sc);
  const int lane_mode = lane_count_mode(sc);
  // speculative placement only with the per-lane LDS dict (MODE 0); the later kernels see the same
  DevSchema scx = sc;
  if (lane_mode != 0 || !fast_ok) scx.spec = nullptr;
  // record-shape templates first (k_tpl_lane, tfrg_tpl.hip): framed records (with CRC verdicts or,
  // kFlagNoCrc, the mask match alone), a schema of <= kLeanMaxSlots slots; k_lane_count then takes
  // only the records it left
  const bool lean = cfg.lean && sc.n_tpl && fast_ok && S <= kLeanMaxSlots && o.lmask && o.rlist &&
                    (sc.tpl_w == 16 || sc.tpl_w == 32 || sc.tpl_w == 64) &&
                    !(b.flags & kFlagPayloadOnly) && b.nbytes < 0xffffff00ull;
  const bool tpl_nocrc = (b.flags & kFlagNoCrc) != 0, tpl_strict = (b.flags & kFlagStrictCrc) != 0;
  // every record of the learning sample took a template and none is above lane_max: the passes after
  // k_tpl_lane (residual lane records, slow walks, large-record CRCs, gathers of placed slots) are
  // usually empty, and a full grid of workgroups that exit at once costs ~4 us per launch; they
  // run with small grids instead (any work they do find is still done: every one strides)
  const bool quiet = lean && cfg.tpl_full && !cfg.body_count;
  // every slot speculatively placed (DevSchema::spec, a target for each)
  bool all_spec = scx.spec && cfg.spec_h && S <= 64;
  for (uint32_t k = 0; all_spec && k < S; ++k) all_spec = cfg.spec_h[k] != 0u;
  // Optimistic: quiet with every slot placed (C1-shaped batches). A batch all of whose records take a
  // template is complete after k_tpl_lane; the passes after it would only launch. The last
  // workgroup of k_tpl_lane does their bookkeeping (tpl_quiet_finish), or flags the batch for a full
  // re-run by the host (tfrg_result_info) if a record took no template. Saves five dependent
  // launches (~4 us each) per batch.
  // (not in strict mode with unchecked-frame templates: their records are errors there, for the full passes)
  const bool quiet_tpl = cfg.optimistic && quiet && all_spec && S > 0 && !(tpl_strict && cfg.tpl_unchecked);
  // Optimistic without record shapes (C2: records above lane_max, every slot one inline value in the
  // learning sample, placed speculatively by k_lane_count MODE 0): k_lane_count, k_tail_count, and
  // the last workgroup of k_tail_count ends the decode (tail_quiet_finish) or flags it for a full
  // re-run. Not in strict mode (a CRC failure withdraws a record's columns).
  const bool quiet_big = cfg.optimistic && !lean && all_spec && S > 0 && lane_mode == 0 && fast_ok &&
                         cfg.body_count && !tpl_strict && b.n > 0;
  cfg.ran_optimistic = quiet_tpl || quiet_big;
  cfg.ran_quiet_big = quiet_big;
  // quiet_big: the records above lane_max walked beside the streaming CRC by k_tail_count's first
  // workgroups (role_big_walk) when its per-lane dicts fit the launch's LDS
  const bool walk_beside = quiet_big && cfg.walk_beside && tail_walk_fits(sc);
  // (optimistic: status / verdict and constant order words are implicit, tfrg_info.implicit_cols;
  // TFRG_IMPLICIT_STATUS says every verdict is 7: CRCs on and every template spec-framed, else
  // k_tpl_lane stores status and verdict per record)
  cfg.implicit = lean && cfg.ran_optimistic ? (!tpl_nocrc && !cfg.tpl_unchecked ? TFRG_IMPLICIT_STATUS : 0u) |
                                                  (cfg.ord_const ? TFRG_IMPLICIT_ORDER : 0u) |
                                                  (cfg.len_const ? TFRG_IMPLICIT_BYTES_LEN : 0u)
                                            : 0u;
  // (and the bytes_off words of a slot at one end-relative offset in every shape, when the caller's
  // u32 ends are on the device to recompute them from: tfrg_info.implicit_off_slots. Every slot of
  // such a decode is placed, so the slot's column rows are n * its rank among the bytes slots)
  cfg.implicit_off = lean && quiet_tpl && b.omode != kOffU64 && !(b.flags & kFlagMaterializeBytes) ? cfg.off_rel : 0ull;
  DevOut ox = o;
  if (!lean) {
    ox.lmask = nullptr;
    ox.rlist = nullptr;
  }
  mark(kStageTplLane);
  if (lean) {
    const LeanArgs a = lean_args(b, sc, o, cfg, scx.spec && cfg.spec_h);
    const hipError_t e = launch_tpl_lane(b, ox, a, sc.tpl_img, sc.tpl_w, cfg.num_cus, st);
    if (e != hipSuccess) return e;
  }
  if (quiet_tpl) return mark_rest(kStageLaneCount);  // (k_tpl_lane's last workgroup finished the decode)
  mark(kStageLaneCount);
  // (after a template pass that took its whole sample the residual pass is usually empty; it
  // strides over whatever groups it finds. Not for records above lane_max: k_tpl_lane leaves
  // every one of them, and walking them is this pass's work)
  launch_lane_count(b, scx, ox, d_tab, cfg, walk_beside, lane_mode, std::min(cfg.lane_grid, quiet ? 64 : cfg.lane_grid), st);
  mark(kStageBodyCount);
  if (cfg.body_count && lane_mode != 0) launch_body_count(b, ox, cfg.num_cus, st);  // (lane modes 1 and 2 only)
  mark(kStageTailCount);
  // the exception paths before the scan, one launch. (A small batch: fewer workgroups -- both roles
  // stride -- so that an empty launch, the usual case of batches of small records, is not a full
  // grid of dispatches; no record above lane_max: role 2 has nothing to stream)
  const uint32_t tail_cap = std::max(8u, (uint32_t)(b.nbytes >> 16) + b.n / 4096u);
  launch_tail_count(b, scx, ox, d_tab, d_consts, cfg, quiet_big, walk_beside,
                    cfg.body_count ? tail_cap : std::min(tail_cap, 32u), st);
  if (quiet_big) return mark_rest(kStageSpine);  // (k_tail_count's last workgroup finished the decode)
  if (cfg.poison[0] != 0xffffffffu && S > 0) launch_poison_loc(ox, b.n, S, cfg.poison, st);
  mark(kStageSpine);
  if (S > 0) launch_spine(ox, scx, n_tiles, b.n, st);
  mark(kStageDownGather);
  if (S > 0) {
    // (at most 8 resident 256-thread workgroups per CU; larger batches stride). Every slot with a
    // speculative target: usually all placed and nothing to do but the launch, one per CU (a failed
    // placement strides over the tiles; a small batch also strides with fewer)
    uint32_t resident = all_spec ? std::min(cus, std::max(8u, n_tiles / 4u)) : 8u * cus;
    if (all_spec && quiet) resident = std::min(resident, 32u);
    launch_down_gather(b, scx, ox, cfg, n_tiles, resident, st);
  }
  mark(kStageTailGather);
  if (S > 0) {  // the gathers after the scan: lane records' lists, staged and huge large records
    // (a small batch: its roles stride over fewer waves; large records keep the full grid)
    int cap = (int)std::min<uint64_t>((uint64_t)cfg.wave_grid,
                                      std::max<uint64_t>(8u, std::max<uint64_t>(b.n / 1024u, b.nbytes >> 16)));
    if (quiet && all_spec) cap = std::min(cap, 32);
    launch_tail_gather(b, scx, ox, cfg, cap, st);
  }
  mark(kStageMaterialize);  // (the caller launches the optional materialize pass and marks the end)
  return hipGetLastError();
}

}  // namespace tfrg
