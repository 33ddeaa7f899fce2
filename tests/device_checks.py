"""Loader of tests/_build/libdbw_device_checks.so (tests/device_checks.hip): the product's shared host+device arithmetic evaluated on the
GPU on caller-supplied operands.  Checker side: built by build.py's build_device_checks (also by __graft_entry__.build()), here on demand."""
import ctypes
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        spec = importlib.util.spec_from_file_location('_dbw_build', os.path.join(HERE, '..', 'differentiable-blocksworld_amd', 'build.py'))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        _LIB = ctypes.CDLL(b.build_device_checks())
        p, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
        _LIB.dbwt_divcheck.argtypes = [p, p, ll, p, p]
        _LIB.dbwt_lane_merge.argtypes = [p, p, p, i, i, p, p, p]
        _LIB.dbwt_model_math.argtypes = [i, p, p, p, i, f, p, p]
        _LIB.dbwt_lds_agg.argtypes = [p, p, p, i, i, i, i, p, p]
        for fn in (_LIB.dbwt_divcheck, _LIB.dbwt_lane_merge, _LIB.dbwt_model_math, _LIB.dbwt_lds_agg):
            fn.restype = i
    return _LIB


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f'{name} failed ({rc})')


LDS_AGG_OPS = ('add', 'add_wave', 'add_wave_merged')


def lds_agg(keys, active, values, n_keys, log2_slots, op, rounds, device='cuda:0'):
    """dbwt_lds_agg on CPU tensors: keys / active (n,) int32, values (n, 3) fp32, n = workgroups * rounds * 256 -> out (n_keys, 3) fp32 on the
    CPU.  Refuses an active key outside [0, n_keys) before anything is launched: the kernel indexes `out` with it."""
    import torch
    n = keys.numel()
    assert n % (rounds * 256) == 0 and active.numel() == n and tuple(values.shape) == (n, 3)
    assert keys.dtype == torch.int32 and active.dtype == torch.int32 and values.dtype == torch.float32
    on = active != 0
    assert bool(((keys[on] >= 0) & (keys[on] < n_keys)).all()), 'active key out of range'
    k_d, a_d, v_d = keys.contiguous().to(device), active.contiguous().to(device), values.contiguous().to(device)
    out = torch.zeros(n_keys, 3, dtype=torch.float32, device=device)
    call('dbwt_lds_agg', k_d.data_ptr(), a_d.data_ptr(), v_d.data_ptr(), n // (rounds * 256), rounds, log2_slots, LDS_AGG_OPS.index(op),
         out.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    return out.cpu()
