"""GPU helper: where a workgroup of scene_bins_kernel spends its time, from a library built with -DDBW_PROFILE_BINS (tools/variants.sh
bprof "-DDBW_PROFILE_BINS"; run with DBW_HIP_LIB=tools/variants/bprof.so): s_memtime deltas of the wave that runs each stage, summed over
the workgroups of one training step, for the scene that goes first in the launch (the blocks) and the other (sky + ground).
usage: bins_cycles.py views H W blocks fpp txt [flags]      (flags: dbw_debug_set_flags)"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
import torch, bench
from dbw_amd import _lib
from dbw_amd.parallel import ShardedTrainStep

class A: pass
args = A(); args.views, args.H, args.W, args.blocks, args.fpp, args.txt = [int(x) for x in sys.argv[1:7]]
flags = int(sys.argv[7], 0) if len(sys.argv) > 7 else 0
dev = torch.device('cuda', 0)
model, inp = bench.build_workload(args, dev)
model.sync_free = True
model.set_cur_epoch(int(os.environ.get('DBW_EPOCH', '0')))
lib = _lib.load()
lib.dbw_debug_set_flags(flags)
step = ShardedTrainStep(model, seed=1)
for _ in range(3):
    step(inp)
torch.cuda.synchronize()
buf = (ctypes.c_ulonglong * 32)()
lib.dbw_debug_read_bins_profile(buf, 1)
step(inp)
torch.cuda.synchronize()
lib.dbw_debug_read_bins_profile(buf, 1)
names = {14: 'extents', 1: 'coarse scan (+ wait for the face range)', 15: 'masks + transposition + barrier (wave 0)', 2: 'masks (wave 0)',
         3: 'transposition (wave 0)', 4: 'prefix + atomics', 5: 'dom (wave 1)', 6: 'fill (wave 0, from the barrier)'}
print(f'views {args.views} {args.H}x{args.W} blocks {args.blocks} flags {flags}')
for s, scene in enumerate(('first scene (blocks)', 'second scene (env)')):
    v = list(buf)[s * 16:(s + 1) * 16]
    wg = max(v[8], 1)
    print(f'  {scene}: {v[8]} workgroups, {v[7] / wg:.0f} ticks each; per workgroup: slots scanned {v[9] / wg:.1f}, entries {v[10] / wg:.1f}; '
          f'bins with an empty list {v[13]}')
    for i, name in names.items():
        print(f'    {name:45s} {v[i] / wg:9.1f} ticks / workgroup  {100.0 * v[i] / max(v[7], 1):5.1f} %')
