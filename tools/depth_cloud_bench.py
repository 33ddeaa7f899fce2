"""Times dbw_lens_depth_cloud alone at N frames of H x W depth samples on a grid of G^3 cells: the analytic capture of
tests/depth_fixture.py (a ground plane and two boxes, cameras on a ring, a mild radial-tangential lens), `--distinct` cameras cast in fp64
and tiled to N frames, every sample valid (edge rule off, the whole 16-bit range, cameras steep enough that a cube of 16 m holds every hit).

The call is made through the binding with every buffer allocated beforehand -- nothing but the library's five kinds of launches is inside a
timed window --, `--repeats` windows of `--inner` calls each after a warm-up, wall clock between device synchronisations.  `--numpy` also
times ops.depth_cloud_host once on the same input and compares the bytes.  `--path hip` runs a warm-up and one window only, for a kernel trace
of its own (rocprofv3 --kernel-trace --stats -- python tools/depth_cloud_bench.py --path hip).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import depth_fixture as DF                                       # noqa: E402
from dbw_amd import _lib, ops                                    # noqa: E402
from dbw_amd.dataset import lens_zoom                            # noqa: E402


def capture(N, H, W, distinct):
    c2w = DF.cameras_gl(distinct, radius=2.5, height=4.0)        # steep enough that every ray meets the ground within 8 m of the origin
    intr = (0.9 * W, 0.92 * W, 0.51 * W, 0.48 * H)
    maps = np.stack([DF.cast(c2w[k], intr, DF.MILD, H, W)[0] for k in range(distinct)])
    ids = np.arange(N) % distinct
    poses = np.stack([np.concatenate([(c2w[k, :3, :3] * np.array([1.0, -1.0, -1.0]) * DF.UNIT).reshape(9), c2w[k, :3, 3]]) for k in ids])
    cams = ops.lens_table(np.tile(np.array(intr), (N, 1)), np.tile(np.array(DF.MILD), (N, 1)), np.zeros(N)).numpy()
    zoom = lens_zoom(H, W, intr, DF.MILD)                        # the target pinhole zoomed until every pixel of it reads inside the source frame
    return np.ascontiguousarray(maps[ids]), cams, ops.lens_target(intr, zoom).numpy(), poses.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--H', type=int, default=192)
    ap.add_argument('--W', type=int, default=256)
    ap.add_argument('--grid', type=int, default=128)
    ap.add_argument('--bound', type=float, default=8.0, help='half-size of the cube in metres (the default holds every sample of the capture)')
    ap.add_argument('--distinct', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--numpy', action='store_true')
    ap.add_argument('--path', choices=['both', 'hip'], default='both')
    args = ap.parse_args()
    dev = torch.device('cuda')
    N, H, W, G = args.frames, args.H, args.W, args.grid
    depth, cams, target, poses = capture(N, H, W, args.distinct)
    box = ops.depth_box(-args.bound, args.bound, G)
    lib = _lib.family('lens')
    d = torch.from_numpy(depth.view(np.int16)).to(dev)
    capacity = min(G ** 3, N * H * W)
    ws = torch.empty(lib.dbw_lens_depth_cloud_workspace_bytes(G), dtype=torch.uint8, device=dev)
    points, counts = torch.empty(capacity, 3, device=dev), torch.empty(capacity, dtype=torch.int32, device=dev)
    info = torch.empty(3, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.call('dbw_lens_depth_cloud', d.data_ptr(), N, H, W, cams.ctypes.data, target.ctypes.data, poses.ctypes.data, box.ctypes.data, G, 1, 65535, 1, 0,
                  1, ws.data_ptr(), points.data_ptr(), counts.data_ptr(), capacity, info.data_ptr(), stream)

    def window(inner):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(inner):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / inner

    window(2)                                                    # warm-up: the library, first launches
    times = [window(args.inner) for _ in range(args.repeats if args.path == 'both' else 1)]
    M, accumulated, outside = [int(v) for v in info.tolist()]
    ts = sorted(times)
    res = {'frames': N, 'H': H, 'W': W, 'grid': G, 'bound_m': args.bound, 'distinct_cameras': args.distinct, 'samples': N * H * W, 'accumulated': accumulated,
           'outside': outside, 'points': M, 'workspace_bytes': ws.numel(), 'device': torch.cuda.get_device_name(0), 'inner_calls': args.inner,
           'runs_ms': [round(t * 1e3, 4) for t in times], 'median_ms': ts[len(ts) // 2] * 1e3, 'min_ms': ts[0] * 1e3, 'max_ms': ts[-1] * 1e3,
           'accumulated_samples_per_s_whole_call': accumulated / ts[len(ts) // 2]}
    if args.numpy:
        t = time.perf_counter()
        p, c, i = ops.depth_cloud_host(depth, cams, target, poses, -args.bound, args.bound, grid=G, return_info=True)
        res['numpy_ms'] = (time.perf_counter() - t) * 1e3
        res['numpy_same_bytes'] = bool(i == [M, accumulated, outside] and p.tobytes() == points[:M].cpu().numpy().tobytes()
                                       and c.tobytes() == counts[:M].cpu().numpy().tobytes())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
