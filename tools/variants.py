#!/usr/bin/env python3
"""Measurement-only builds of libtfrg (never the product library): the kernel sources copied to a
temporary directory, patched, built into tfr_reader/libtfrg_<name>.so (load with TFRG_LIB=...), for
paired A/Bs on the GPU box (tools/ab.sh). Patches are (file, old, new) string replacements; a
variant whose patch no longer applies is an error (tests/test_variants_apply.py checks every one).
usage: variants.py name [name ...]"""
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
CS = REPO / "tfrecords-reader_amd" / "csrc"

VARIANTS = {
    # k_tpl_lane printing every record it leaves to k_lane_count (debug)
    "dbgtpl": [("tfrg_tpl.hip", "#include <hip/hip_runtime.h>", "#define TFRG_DEBUG_TPL 1\n#include <hip/hip_runtime.h>")],
    # k_tpl_lane at 8 waves/SIMD (64 VGPRs)
    "lb8v3": [("tfrg_tpl.hip", "__launch_bounds__(kTplBlock, W == 16 ? 6 : (W == 32 ? 4 : 2))",
               "__launch_bounds__(kTplBlock, W == 16 ? 8 : (W == 32 ? 4 : 2))")],
    # k_tail_count in 1024-thread workgroups, one per CU (the streaming CRC's 70 KiB of LDS tables
    # loaded 256 times instead of 512; the same 16 waves per CU)
    "tail1024": [("tfrg_kernels.hip", "constexpr uint32_t kTailBlock = 512;", "constexpr uint32_t kTailBlock = 1024;"),
                 ("tfrg_kernels.hip", "__global__ __launch_bounds__(kTailBlock, 2) void k_tail_count",
                  "__global__ __launch_bounds__(kTailBlock, 4) void k_tail_count")],
    # k_tpl_lane window loads with the streaming (slc) cache policy
    "ntload": [("tfrg_tpl.hip", "__builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + 16u * q, 0, 0)",
                "__builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + 16u * q, 0, 2)")],
    # k_tail_count without role 1 (the exact walker): the streaming CRC's registers alone (timing only)
    "crc_only": [("tfrg_kernels.hip", "  role_slow_count<1, COMPAT, GORD, kTailBlock>(B, sc, o, crc_tab, lane_max);\n", "")],
    # k_tpl_lane at 8 waves/SIMD (64 VGPRs: 4 workgroups per CU instead of 3; spills a few registers)
    "lb8": [("tfrg_tpl.hip", "__launch_bounds__(kTplBlock, W == 16 ? 6 : (W == 32 ? 4 : 2))",
             "__launch_bounds__(kTplBlock, W == 16 ? 8 : (W == 32 ? 4 : 2))")],
    # k_tail_gather without the float copies / the packed int64 decode / int64_ring's pass B
    # (VALU attribution by PMC; wrong results)
    "g_nofloat": [("tfrg_kernels.hip", "  uint64_t m = __ballot(isf);", "  uint64_t m = 0;")],
    "g_noint64": [("tfrg_kernels.hip", "  int rr = int64_ring<COMPAT>(fs, o, iv, bo, bl, cnt, dst, lane, ring);", "  int rr = 1;")],
    "g_nopassb": [("tfrg_kernels.hip", "    while (gtot - gb >= 64u) pass_b(64u);\n", "    gb = gtot;\n"),
                  ("tfrg_kernels.hip", "  if (gtot > gb) pass_b(gtot - gb);", "  gb = gtot;")],
    # int64_ring pass A: a body's byte mask in a dword from saturating subtractions
    "c3bm": [("tfrg_kernels.hip",
              "      const uint32_t lo = sbs > Q ? sbs - Q : 0u, hi0 = sbe > Q ? sbe - Q : 0u, hi = hi0 < 4u ? hi0 : 4u;\n"
              "      if (hi > lo) {  // (1 <= hi <= 4, lo <= 3: both shifts below 32)\n"
              "        bm = (0xffffffffu >> (32u - 8u * hi)) & (0xffffffffu << (8u * lo));\n",
              "      const uint32_t lo = __builtin_elementwise_sub_sat(sbs, Q), hi0 = __builtin_elementwise_sub_sat(sbe, Q), hi = hi0 < 4u ? hi0 : 4u;\n"
              "      if (hi > lo) {\n"
              "        bm = ~(0xfffffffeu << (8u * hi - 1u)) & (0xffffffffu << (8u * lo));\n")],
    # k_spine without its every-slot-placed fast path (the per-slot fast path and last-workgroup pass)
    "noallp": [("tfrg_scan.hip", "  const bool allp = spec && n_slots <= (uint32_t)kSpineBlock &&",
                "  const bool allp = false && spec && n_slots <= (uint32_t)kSpineBlock &&")],
    # k_down_gather's placed-slot mask by one thread per workgroup, slot after slot
    "serialpm": [("tfrg_scan.hip",
                  "  const uint64_t pmask = sc.spec ? (uint64_t)__ballot(lane < S && spec_placed(sc.spec, o, lane)) : 0ull;\n",
                  "  uint64_t pmask = 0;\n  if (sc.spec)\n    for (uint32_t k = 0; k < S && k < 64u; ++k) pmask |= (uint64_t)spec_placed(sc.spec, o, k) << k;\n"
                  "  pmask = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(pmask >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)pmask);\n")],
    # k_tpl_lane ablations (timing only, wrong results): no template match / no slot extraction and
    # column stores
    "abl_nomatch": [('tfrg_tpl.hip', '        diff |= ((w[4 * q] ^ bm.x) & mm.x) | ((w[4 * q + 1] ^ bm.y) & mm.y) | ((w[4 * q + 2] ^ bm.z) & mm.z) |\n                ((w[4 * q + 3] ^ bm.w) & mm.w);', '        diff |= 0u * (bm.x & mm.x);')],
    "abl_noslot": [('tfrg_tpl.hip', '    if (__ballot(hit)) {\n      const uint32_t* ts', '    if (__ballot(hit) && A.n_slots == 12345u) {\n      const uint32_t* ts')],
    # k_tpl_lane at 7 waves/SIMD (72 VGPRs)
    "lb7": [("tfrg_tpl.hip", "__launch_bounds__(kTplBlock, W == 16 ? 6 : (W == 32 ? 4 : 2))",
             "__launch_bounds__(kTplBlock, W == 16 ? 7 : (W == 32 ? 4 : 2))")],
    # the streaming CRC without its per-record flush (timing only, wrong verdicts)
    "flush_none": [("tfrg_kernels.hip", "                                       uint32_t n_slots, uint32_t lane) {\n  const uint64_t bas = rl64(w.base, k);",
                    "                                       uint32_t n_slots, uint32_t lane) {\n  if (n_slots != 0xfffffffeu) return;\n  const uint64_t bas = rl64(w.base, k);")],
}


# (measurement only) the streaming CRC's loads and group structure without its arithmetic: what the
# role-2 load pattern achieves on its own (wrong verdicts)
VARIANTS["crc_loadonly"] = [("tfrg_kernels.hip", """  auto process = [&](const Grp& g) {
""", """  auto process = [&](const Grp& g) {
    if (n_slots != 0xfffffffeu) {
#pragma unroll
      for (int d = 0; d < kCrcDepth; ++d) S ^= g.wd[d].x ^ g.wd[d].y ^ g.wd[d].z ^ g.wd[d].w;
      return;
    }
""")]


# (measurement) streaming-CRC groups that never cross a record (a record's last group is partial;
# its unused loads repeat the group's last chunk instead of reading ahead)
VARIANTS["crc_align"] = [("tfrg_kernels.hip", """    if (!g.n) return;
    const uint64_t rl = Rs + g.n - 1u;
    const uint32_t k0 = (uint32_t)__popcll(__ballot(w.base <= Rs)) - 1u;
    const uint32_t kl = (uint32_t)__popcll(__ballot(w.base <= rl)) - 1u;""", """    if (!g.n) return;
    const uint32_t k0 = (uint32_t)__popcll(__ballot(w.base <= Rs)) - 1u;
    {
      const uint64_t re = rl64(w.base, k0 + 1u);
      if (Rs + g.n > re) g.n = (uint32_t)(re - Rs);
    }
    const uint64_t rl = Rs + g.n - 1u;
    const uint32_t kl = k0;"""),
    ("tfrg_kernels.hip", """        g.wd[d] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(brs, vo + 1024u * d, 0, 0));""",
     """        g.wd[d] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(brs, vo + 1024u * ((uint32_t)d < g.n ? (uint32_t)d : g.n - 1u), 0, 0));""")]


def build(name: str) -> Path:
    with tempfile.TemporaryDirectory() as td:
        d = Path(td) / "pkg" / "csrc"  # (the sources include ../../include)
        shutil.copytree(CS, d, ignore=shutil.ignore_patterns("build*"))
        (Path(td) / "include").symlink_to(REPO / "include")
        for f, old, new in VARIANTS[name]:
            src = (d / f).read_text()
            assert src.count(old) == 1, (name, f, old[:60])
            (d / f).write_text(src.replace(old, new))
        out = REPO / "tfrecords-reader_amd" / "tfr_reader" / f"libtfrg_{name}.so"
        subprocess.run(["make", "-j8", f"OUT={out}", f"PYMOD={Path(td) / 'unused.so'}", f"{out}"], cwd=d, check=True,
                       stdout=subprocess.DEVNULL)
    return out


if __name__ == "__main__":
    for n in sys.argv[1:]:
        print(build(n))
