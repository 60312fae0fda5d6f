"""Registers the bounds build of csrc/wh_psola.hip (wh_psola) with tests/_variants.py from outside: "psola_bounds"
recompiles wh_api and wh_psola with -DWH_BOUNDS=1.  Imported by __graft_entry__.build() before _variants.ensure(), so that
the variant is built with the others and travels with the tree, and by tests/test_hip_psola_bounds.py before
report_fixture is used.  No pytest and no GPU at import."""
try:  # (as tests._psola_variant from __graft_entry__, by its plain name from the tests: the same table either way)
    from . import _variants
except ImportError:
    import _variants

NAME = "psola_bounds"
_variants.VARIANTS.setdefault(NAME, _variants._checked("wh_psola"))
