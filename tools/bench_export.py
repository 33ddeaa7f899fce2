"""Time of the 8-bit view pipeline (renderer.render_views_u8: lit kernel, dbw_frames_u8, 3 B/pixel copied to a pinned buffer on a second
stream) against the fp32 one followed by the reference's conversion on the host (renderer.render_views, 16 B/pixel through a synchronous
.cpu() per 10 views, then clamp * 255 -> uint8 as utils/image.py:98 does).  Joined scene (sky dome, ground, blocks) of BASELINE config 2:
240 views of 300x400, 10 blocks with 256x256 textures, the model's unlit renderer.  Both warmed up, alternating in one process, wall clock
around a device synchronise, --reps repetitions.  Prints one JSON line.

--once: a few conversions of each kind and one pipeline call, no timing (for a rocprofv3 --kernel-trace --stats run of its own).
--quali DIR: instead, one full qualitative_eval(NV=--views) over 10 inputs into DIR, with its render / encode split."""
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
    ap.add_argument('--views', type=int, default=240)
    ap.add_argument('--H', type=int, default=300)
    ap.add_argument('--W', type=int, default=400)
    ap.add_argument('--blocks', type=int, default=10)
    ap.add_argument('--txt', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--quali', default=None)
    args = ap.parse_args()
    import dbw_amd
    from dbw_amd import mesh as M
    from dbw_amd import ops
    from dbw_amd import renderer as RN
    from bench import make_cfg
    dev = 'cuda:0'
    H, W = args.H, args.W
    torch.manual_seed(227391)
    model = dbw_amd.create_model(make_cfg(args.blocks, 10, args.txt), (H, W)).to(dev).eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(99)
        model.alpha_logit.add_(2.0)
        model.textures.add_(torch.randn(model.textures.shape, generator=g).to(dev))
    R0, T0, K = [t.to(dev) for t in M.synthetic_cameras(10, R_world=model.R_world[0])]
    model._ensure_cameras({'imgs': torch.zeros(1, 3, H, W, device=dev), 'K': K})
    if args.quali:
        imgs = torch.rand(10, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
        loader = [({'imgs': imgs[i:i + 5], 'R': R0[i:i + 5], 'T': T0[i:i + 5], 'K': K[i:i + 5]}, None) for i in (0, 5)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        spent = model.qualitative_eval(loader, dev, path=args.quali, NV=args.views)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        n_files = sum(len(f) for _, _, f in os.walk(args.quali))
        print(json.dumps({'qualitative_eval_s': round(total, 2), 'render_convert_copy_s': round(spent['render'], 2),
                          'file_encoding_s': round(spent['encode'], 2), 'files': n_files, 'NV': args.views, 'inputs': 10}))
        return
    with torch.no_grad(), model._host_packed_rebuild():
        scene = model.build_scene(filter_transparent=True)
    R = (R0[:1] @ RN.get_circle_traj(N_views=args.views)[0].to(dev)).contiguous()
    T = T0[:1].expand(args.views, -1).contiguous()
    r = model.renderer
    out = torch.empty(args.views, H, W, 3, dtype=torch.uint8, pin_memory=True)

    def new_path():
        return RN.render_views_u8(scene, R, T, renderer=r, out=out)

    def parent_path():
        x = RN.render_views(scene, R, T, renderer=r)                                       # (N,3,H,W) fp32 on the host
        return (x * 255).permute(0, 2, 3, 1).clamp(0, 255).numpy().astype('uint8')        # utils/image.py:98

    def parent_render_only():
        return RN.render_views(scene, R, T, renderer=r)

    img = r.render_viz(scene, R[:10], T[:10])
    bkg = torch.rand(3, H, W, device=dev)
    if args.once:
        new_path()
        for _ in range(20):
            ops.frames_u8(img)
            ops.frames_u8(img, bkg=bkg)
        torch.cuda.synchronize()
        print(json.dumps({'once': True, 'faces': int(scene.faces.shape[0]), 'frames_per_conversion': 10}))
        return
    paths = {'u8_pipeline': new_path, 'fp32_then_host_conversion': parent_path, 'fp32_views_only': parent_render_only}
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, fn in paths.items():                 # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    # the render alone (no conversion, no copy), for the split
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    B = RN._views_per_chunk(scene, (H, W), args.views)
    for k in range(0, args.views, B):
        r.render_viz(scene, R[k:k + B], T[k:k + B])
    torch.cuda.synchronize()
    render_only = time.perf_counter() - t0
    print(json.dumps({'workload': f'{args.views} views {H}x{W}, {args.blocks} blocks, {int(scene.faces.shape[0])} faces, 4x super-sampling',
                      'seconds': {k: [round(x, 4) for x in v] for k, v in times.items()},
                      'median_s': {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()},
                      'spread_s': {k: round(max(v) - min(v), 4) for k, v in times.items()},
                      'lit_render_only_s': round(render_only, 4), 'views_per_chunk': B,
                      'device_to_host_bytes': {'u8_pipeline': 3 * H * W * args.views, 'fp32': 16 * H * W * args.views}}))


if __name__ == '__main__':
    main()
