"""tools/variants.py patches the kernel sources by exact string: every patch of every variant must
find its `old` string exactly once in the file it names, in the file as committed and in the file
as the variant's earlier patches leave it, which is what variants.py applies it to (no compile)."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tfrecords-reader_amd" / "csrc"


def _variants():
    spec = importlib.util.spec_from_file_location("tfrg_variants", ROOT / "tools" / "variants.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.VARIANTS


VARIANTS = _variants()


def test_there_are_variants():
    assert VARIANTS


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variant_patches_apply_exactly_once(name):
    sources = {}
    for fname, old, new in VARIANTS[name]:
        assert (CSRC / fname).is_file(), f"{name}: no source file {fname}"
        pristine = (CSRC / fname).read_text()
        assert pristine.count(old) == 1, f"{name}: {fname} holds {pristine.count(old)} copies of {old[:60]!r}"
        src = sources.setdefault(fname, pristine)
        assert src.count(old) == 1, f"{name}: {fname} holds {src.count(old)} copies of {old[:60]!r}"
        assert new != old
        # (the patches of one variant are applied in order: the next one sees this one's result)
        sources[fname] = src.replace(old, new)
