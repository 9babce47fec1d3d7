"""The ctypes mirror of tfrg_select_term (tfr_reader/_native.py) has the layout include/tfrg.h gives
it (the method of tests/test_abi_layout.py), the TFRG_SEL_* constants of the header are the binding's,
and the two new entry points are declared on both sides."""

import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from tfr_reader import _native as N

INCLUDE = Path(__file__).resolve().parents[1] / "include"
STRUCTS = {"tfrg_select_term": N.TfrgSelectTerm}
CONSTANTS = {"TFRG_SEL_MAX_TERMS": N.SEL_MAX_TERMS, "TFRG_SEL_VALUE": N.SEL_VALUE, "TFRG_SEL_ANY": N.SEL_ANY,
             "TFRG_SEL_COUNT": N.SEL_COUNT, "TFRG_SEL_BYTES_LEN": N.SEL_BYTES_LEN, "TFRG_SEL_STATUS": N.SEL_STATUS,
             "TFRG_SEL_EQ": N.SEL_EQ, "TFRG_SEL_NE": N.SEL_NE, "TFRG_SEL_LT": N.SEL_LT, "TFRG_SEL_LE": N.SEL_LE,
             "TFRG_SEL_GT": N.SEL_GT, "TFRG_SEL_GE": N.SEL_GE, "TFRG_SEL_APPEND": N.SEL_APPEND}


def _c_layout(tmp_path: Path) -> dict:
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tfrg.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'  printf("{cname} {fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname}*)0)->{fname}));')
    for name in CONSTANTS:
        lines.append(f'  printf("const {name} %lld 0\\n", (long long)({name}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(INCLUDE), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    res: dict = {}
    for line in out.splitlines():
        parts = line.split()
        if parts[1] == "size":
            res[(parts[0], "__size__")] = int(parts[2])
        else:
            res[(parts[0], parts[1])] = (int(parts[2]), int(parts[3]))
    return res


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_select_term_matches_the_header(tmp_path):
    c = _c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert c[(cname, "__size__")] == C.sizeof(py) == 32, cname
        for fname, _ in py._fields_:
            f = getattr(py, fname)
            assert c[(cname, fname)] == (f.offset, f.size), (cname, fname)
    for name, value in CONSTANTS.items():
        assert c[("const", name)][0] == value, name


def test_every_header_field_is_mirrored():
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / "tfrg.h").read_text(), flags=re.S)
    for cname, py in STRUCTS.items():
        m = re.search(r"typedef struct " + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", text, flags=re.S)
        assert m, cname
        names = re.findall(r"\b(\w+)\s*(?:\[\s*\d+\s*\])?\s*;", m.group(1))
        assert names == [f for f, _ in py._fields_], (cname, names)
    for fn in ("tfrg_result_select_rows", "tfrg_ctx_set_select_tile"):
        assert re.search(r"\bint " + fn + r"\(", text) and fn in N.SIGNATURES, fn
        assert hasattr(N.lib(), fn)
    assert len(N.SIGNATURES["tfrg_result_select_rows"][1]) == 14
