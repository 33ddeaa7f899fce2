"""Time of the lit 4x visualisation render (Renderer(shading_type='flat' | 'phong').render_packed(viz_purpose=True): one forward-only
kernel that resolves its 4x4 super-samples in registers) against the unlit visualisation render of the same scene and views
(Renderer.render_packed(viz_purpose=True) of a 'raw' renderer: the training forward at 4x, fragments stored, then avg_pool2d).
Blocks scene of BASELINE config 2: 49 views, 300x400, 10 blocks with 256x256 textures.  Both warmed up, alternating in one process, each
repetition timed over >= --seconds ending in a synchronise.  Prints one JSON line.  --once: a few calls of each and no timing (for a
rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
sys.path.insert(0, ROOT)

import torch                                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--H', type=int, default=300)
    ap.add_argument('--W', type=int, default=400)
    ap.add_argument('--blocks', type=int, default=10)
    ap.add_argument('--txt', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=2.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    import dbw_amd
    from dbw_amd import mesh as M
    from dbw_amd.renderer import DIRECTION_LIGHT, Renderer
    from bench import make_cfg
    dev = 'cuda:0'
    torch.manual_seed(227391)
    model = dbw_amd.create_model(make_cfg(args.blocks, 10, args.txt), (args.H, args.W)).to(dev).eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(99)
        model.alpha_logit.add_(2.0)
        model.textures.add_(torch.randn(model.textures.shape, generator=g).to(dev))
    R, T, K = [t.to(dev) for t in M.synthetic_cameras(args.views, R_world=model.R_world[0])]
    model._ensure_cameras({'imgs': torch.zeros(1, 3, args.H, args.W, device=dev), 'K': K})
    with torch.no_grad(), model._host_packed_rebuild():
        scene = model.build_blocks_scene(filter_transparent=True)
    light = {'name': 'directional', 'direction': [DIRECTION_LIGHT], 'ambient_color': [[0.7] * 3], 'diffuse_color': [[0.4] * 3], 'specular_color': [[0.] * 3]}
    base = {**model.renderer.init_kwargs, 'background_color': (1, 1, 1), 'faces_per_pixel': 1, 'sigma': 0, 'detach_bary': False}
    renderers = {'unlit': Renderer(model.img_size, **base), 'flat': Renderer(model.img_size, **{**base, 'lights': light, 'shading_type': 'flat'}),
                 'phong': Renderer(model.img_size, **{**base, 'lights': light, 'shading_type': 'phong'})}
    for r in renderers.values():
        r.update_cameras(device=dev, K=model.renderer.cameras.K)

    def call(name):
        with torch.no_grad():
            return renderers[name].render_packed(scene, R, T, viz_purpose=True)

    for name in renderers:                       # warm-up
        for _ in range(3):
            call(name)
    torch.cuda.synchronize()
    if args.once:
        print(json.dumps({'once': True, 'faces': int(scene.faces.shape[0])}))
        return
    times = {name: [] for name in renderers}
    for _ in range(args.reps):
        for name in renderers:                   # alternating
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(5):
                    call(name)
                n += 5
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.seconds:
                    break
            times[name].append(dt / n * 1e3)
    out = {'workload': f'{args.views} views {args.H}x{args.W}, {args.blocks} blocks, {int(scene.faces.shape[0])} faces, 4x super-sampling',
           'ms_per_call': {k: [round(x, 4) for x in v] for k, v in times.items()},
           'median_ms': {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()},
           'spread_ms': {k: round(max(v) - min(v), 4) for k, v in times.items()},
           'bytes_written_per_view': 16 * args.H * args.W}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
