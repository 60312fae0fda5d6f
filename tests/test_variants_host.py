"""CPU: the variant table of tests/_variants.py names real translation units and instruments what a bounds variant needs.
A typo there otherwise shows up only as a failed hipcc line when the variants are built."""
import os

import _variants as V

CHECKED = [n for n in V.VARIANTS if n == "bounds" or n.endswith("_bounds")]


def test_every_translation_unit_exists():
    missing = [(n, tu) for n, tus in V.VARIANTS.items() for tu in tus
               if not os.path.isfile(os.path.join(V.PKG, "csrc", tu + ".hip"))]
    assert missing == []


def test_bounds_variants_instrument_wh_api_and_every_unit_they_name():
    assert len(CHECKED) == len(V.VARIANTS) - 1
    for n in CHECKED:
        assert "wh_api" in V.VARIANTS[n], n  # wh_bounds_build() and the record readers live there
        assert all("-DWH_BOUNDS=1" in flags for flags in V.VARIANTS[n].values()), n


def test_paths_are_distinct_files_under_lib_variants():
    paths = [V.path(n) for n in V.VARIANTS]
    assert len(set(paths)) == len(paths)
    assert all(os.path.dirname(p) == os.path.join(V.PKG, "lib", "variants") for p in paths)


def test_spec_is_what_build_variants_takes():
    assert V.spec("dtw_bounds") == "dtw_bounds=wh_api:-DWH_BOUNDS=1;wh_dtw:-DWH_BOUNDS=1"
