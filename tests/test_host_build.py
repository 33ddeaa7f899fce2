"""CPU: tests/host_build.py decides staleness from every header of csrc/, the transitive ones included."""
import os

import host_build


def test_host_lib_rebuilds_after_any_csrc_header_and_not_otherwise():
    """icp_math.h reaches raster_math.h only through model_math.h: a raster_math.h newer than libhost_icp_math.so compiles it again, and a
    second call without that does not.  (The header's own times are put back: the product library depends on them too.)"""
    so = os.path.join(host_build.HERE, '_build', 'libhost_icp_math.so')
    header = os.path.join(host_build.CSRC, 'raster_math.h')
    lib = host_build.host_lib('icp_math')
    built = os.stat(so).st_mtime_ns
    assert host_build.host_lib('icp_math') is lib and os.stat(so).st_mtime_ns == built
    before = os.stat(header)
    try:
        os.utime(header, ns=(before.st_atime_ns, built + 1_000_000))      # what `touch` does, to the millisecond behind the library
        assert host_build.host_lib('icp_math') is lib                     # (one CDLL per stem)
        assert os.stat(so).st_mtime_ns > built + 1_000_000
    finally:
        os.utime(header, ns=(before.st_atime_ns, before.st_mtime_ns))
    rebuilt = os.stat(so).st_mtime_ns
    host_build.host_lib('icp_math')
    assert os.stat(so).st_mtime_ns == rebuilt
