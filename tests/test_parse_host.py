"""CPU tests of the scene parsing entry points' host side (include/dbw_viz.h: dbw_viz_parse_fwd, dbw_viz_parse_workspace_bytes): every
argument is validated before any launch -- the calls below hand over pointers that must never be dereferenced on the device -- and the
Python layers above refuse what they cannot do.  The boundary itself (header, ctypes table, exported symbols): tests/test_abi_families.py."""
import ctypes

import numpy as np
import pytest
import torch

import dbw_amd
from dbw_amd import _lib, ops
from dbw_amd.renderer import Renderer

F = 4


def _args(**over):
    """Arguments of dbw_viz_parse_fwd with every required pointer non-null and a valid host copy of the labels."""
    p = ctypes.c_void_p(256)
    host = over.pop('labels', [0, 1, 63, 2])
    keep = np.ascontiguousarray(host, np.int32)
    a = dict(face_verts_c=p, first_idx=p, num_faces=p, neighbor=p, c2o=p, Fc_stride=2 * F, N=1, F_total=2 * F, H=4, W=4, F=F, perspective_correct=1,
             face_label=p, face_label_host=ctypes.c_void_p(keep.ctypes.data), label=p, depth=p, cover=p, counts=p, workspace=p,
             workspace_bytes=1 << 30, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values()), keep


def _call(**over):
    lib = _lib.family('viz')
    args, keep = _args(**over)
    rc = lib.dbw_viz_parse_fwd(*args)
    return rc, lib.dbw_last_error()


def test_parse_entry_point_validates_before_any_launch():
    for name in ('face_verts_c', 'first_idx', 'num_faces', 'face_label', 'label', 'depth', 'cover', 'counts', 'workspace'):
        rc, err = _call(**{name: None})
        assert rc == -1 and b'null pointer' in err, name
    for name in ('N', 'H', 'W'):
        for bad in (0, -3):
            rc, err = _call(**{name: bad})
            assert rc == -1 and b'bad size' in err, (name, bad)
    rc, err = _call(F=0)
    assert rc == -1 and b'bad size' in err
    rc, err = _call(F_total=-1)
    assert rc == -1 and b'bad size' in err
    rc, err = _call(workspace_bytes=64)
    assert rc == -1 and b'workspace too small' in err
    lib = _lib.family('viz')
    need = lib.dbw_viz_parse_workspace_bytes(2 * F, 1, F, 4, 4)
    rc, err = _call(workspace_bytes=need - 1)
    assert rc == -1 and b'workspace too small' in err
    # a label outside [0, 64), on the host copy
    for labels, where in (([0, 1, 64, 2], b'face_label[2] = 64'), ([-1, 1, 63, 2], b'face_label[0] = -1'), ([0, 1, 2, 255], b'face_label[3] = 255')):
        rc, err = _call(labels=labels)
        assert rc == -1 and where in err and b'outside [0, 64)' in err, labels
    with pytest.raises(RuntimeError, match=r'face_label\[2\] = 64'):
        _lib.call('dbw_viz_parse_fwd', *_args(labels=[0, 1, 64, 2])[0])


def test_parse_workspace_bytes():
    lib = _lib.family('viz')
    # 0 for arguments the call would refuse
    for bad in ((-1, 1, 4, 4, 4), (8, 0, 4, 4, 4), (8, -1, 4, 4, 4), (8, 1, 0, 4, 4), (8, 1, 4, 0, 4), (8, 1, 4, 4, 0), (8, 1, 4, 4, -2),
                (1 << 27, 1, 4, 4, 4), (8, 1, 4, 1 << 24, 4)):
        assert lib.dbw_viz_parse_workspace_bytes(*bad) == 0, bad
    # the rasteriser's binned workspace plus one label per clipped face
    base = lib.dbw_rasterize_workspace_bytes_binned(100, 2, 40, 56)
    got = lib.dbw_viz_parse_workspace_bytes(100, 2, 50, 40, 56)
    assert got >= base + 400 and got % 256 == 0 and got - base < 400 + 256
    assert lib.dbw_viz_parse_workspace_bytes(100000, 2, 50000, 40, 56) - lib.dbw_rasterize_workspace_bytes_binned(100000, 2, 40, 56) >= 400000


def test_python_layers_refuse_what_they_cannot_do():
    assert _lib.VIZ_MAX_LABELS == 64 and _lib.VIZ_NO_LABEL == 255 and _lib.VIZ_ABI_VERSION == 1        # additive: the revision stays
    r = Renderer((8, 8))
    with pytest.raises(NotImplementedError, match='perspective cameras'):
        r.parse_packed(None, [0], torch.eye(3)[None], torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        ops.parse_scene(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), [0], torch.eye(3)[None], torch.zeros(1, 3), torch.eye(4),
                        ops.RenderCfg(8, 8, 1, 0.0, 0.001, True, False, 1))
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': 63, 'txt_size': 8},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001}}}
    m = dbw_amd.create_model(cfg, (16, 24))
    with pytest.raises(NotImplementedError, match='64 bits'):
        m.parse_views(dict(imgs=torch.zeros(1, 3, 16, 24), R=torch.eye(3)[None], T=torch.zeros(1, 3)))
    # the new arguments default to off
    import inspect
    from dbw_amd.trainer import Trainer
    assert inspect.signature(m.qualitative_eval).parameters['parse'].default is False
    sig = inspect.signature(Trainer.evaluate).parameters
    assert sig['parse'].default is False and sig['masks'].default is None
