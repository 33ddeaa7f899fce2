"""The per-source compiler flags of the library build (no GPU, no compiler run)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    spec = importlib.util.spec_from_file_location('_dbw_build_flags', os.path.join(ROOT, 'differentiable-blocksworld_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_render_sources_are_built_without_slp_packing_and_nothing_else_is():
    b = _build()
    assert set(b.NO_SLP) <= set(b.SOURCES)
    for s in b.SOURCES:
        f = b.flags_for(s)
        assert ('-fno-slp-vectorize' in f) == (s in b.NO_SLP), s
        assert f[:len(b.FLAGS)] == b.FLAGS, s              # the parity flags stay on every source
    assert '-ffp-contract=off' in b.FLAGS
    assert '-fno-slp-vectorize' not in b.FLAGS               # (tests/device_checks.hip and the other sources keep the default)
