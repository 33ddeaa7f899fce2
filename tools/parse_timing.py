"""Timing of the scene parsing pass (dbw_viz_parse_fwd) next to the K = 1 hard fragment pass (dbw_rasterize_fwd, K = 1) on the same
projected scene: DESIGN.md 6k, profiles/scene_parse.md.  Default: 49 views of 300 x 400, 10 blocks, sky and ground, cameras at 8 degrees.

Both calls run on buffers allocated once, from the same clip tables (project_clip is outside the window).  HIP events around batches of
`--calls` calls, the two passes alternating batch by batch, `--rounds` batches each after `--warmup`; the host's enqueue time per call is
printed next to the device time, because a window whose enqueue time is not well below its device time measures the host.  One JSON line.

    python tools/parse_timing.py [--views 49 --size 300 400 --blocks 10 --rounds 30 --calls 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'differentiable-blocksworld_amd'), os.path.join(ROOT, 'oracle')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch                                                   # noqa: E402
import oracle as O                                             # noqa: E402
import dbw_amd                                                 # noqa: E402
from dbw_amd import _lib, ops                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--size', type=int, nargs=2, default=(300, 400))
    ap.add_argument('--blocks', type=int, default=10)
    ap.add_argument('--elev', type=float, default=8.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = 'cuda:0'
    H, W = a.size
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': a.blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 6, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'kill_blocks': True, 'decouple_rendering': True}}}
    torch.manual_seed(227391)
    model = dbw_amd.create_model(cfg, (H, W))
    with torch.no_grad():
        model.alpha_logit.fill_(2.0)
    model = model.to(dev).eval()
    R, T, Km = O.synthetic_cameras(a.views, R_world=O.world_rotation(115, 0, 0), elev_deg=a.elev)
    R, T, Kmat = R.to(dev), T.to(dev), Km[0].to(dev).contiguous()
    with torch.no_grad(), model._host_packed_rebuild():
        scene = model.build_scene(filter_transparent=True)
    N, F_ = a.views, scene.faces.shape[0]
    cl = ops.project_clip(scene.verts, scene.faces, R, T, Kmat, 1e-8, 0.001, True)
    fvc = cl['face_verts'].view(-1, 3, 3)
    Ft = fvc.shape[0]
    lib = _lib.family('viz')
    s = torch.cuda.current_stream().cuda_stream
    p = ops._ptr

    host = torch.cat([torch.zeros(model.bkg_n_faces), torch.ones(model.ground_n_faces),
                      (2 + torch.arange(a.blocks)).repeat_interleave(model.BNF)]).to(torch.int32).contiguous()
    lab = host.to(dev)
    ws_p = lib.dbw_viz_parse_workspace_bytes(Ft, N, F_, H, W)
    ws_parse = torch.empty(ws_p // 4 + 1, dtype=torch.float32, device=dev)
    label, depth = torch.empty(N, H, W, dtype=torch.uint8, device=dev), torch.empty(N, H, W, dtype=torch.float32, device=dev)
    cover, counts = torch.empty(N, H, W, dtype=torch.int64, device=dev), torch.empty(N, 64, 2, dtype=torch.int32, device=dev)

    def parse():
        _lib.call('dbw_viz_parse_fwd', p(fvc), p(cl['first_idx']), p(cl['num_faces']), p(cl['neighbor']), p(cl['c2o']), 2 * F_, N, Ft, H, W, F_, 1,
                  p(lab), p(host), p(label), p(depth), p(cover), p(counts), p(ws_parse), ws_p, s)

    ws_r = lib.dbw_rasterize_workspace_bytes_binned(Ft, N, H, W)
    ws_raster = torch.empty(ws_r // 4 + 1, dtype=torch.float32, device=dev)
    p2f, zbuf = torch.empty(N, H, W, 1, dtype=torch.int32, device=dev), torch.empty(N, H, W, 1, dtype=torch.float32, device=dev)
    bary, dists = torch.empty(N, H, W, 1, 3, dtype=torch.float32, device=dev), torch.empty(N, H, W, 1, dtype=torch.float32, device=dev)
    nb = cl['neighbor'].view(-1)

    def k1():
        _lib.call('dbw_rasterize_fwd', p(fvc), p(cl['first_idx']), p(cl['num_faces']), p(nb), N, Ft, H, W, 1, 0.0, 1, 1, 0, p(p2f), p(zbuf), p(bary),
                  p(dists), p(ws_raster), ws_r, s)

    def window(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        host_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls, host_s * 1e3 / a.calls

    for _ in range(a.warmup):
        window(parse), window(k1)
    times = {'parse': [], 'k1': []}
    for _ in range(a.rounds):
        times['parse'].append(window(parse))
        times['k1'].append(window(k1))
    # the two passes see the same picture
    c2o = cl['c2o'].view(-1)
    same = bool(torch.equal(label, torch.where(p2f[..., 0] >= 0, lab[c2o[p2f[..., 0].clamp(min=0).long()].long()], torch.tensor(255, device=dev)).to(torch.uint8))
                and torch.equal(depth, zbuf[..., 0]))

    def stats(rows):
        d, h = [r[0] for r in rows], [r[1] for r in rows]
        return {'device_ms_median': round(statistics.median(d), 4), 'device_ms_min': round(min(d), 4), 'device_ms_max': round(max(d), 4),
                'host_enqueue_ms_median': round(statistics.median(h), 4)}

    out = {'what': 'dbw_viz_parse_fwd vs dbw_rasterize_fwd K=1, per call, HIP events', 'views': N, 'H': H, 'W': W, 'blocks': a.blocks, 'faces': F_,
           'elev_deg': a.elev, 'rounds': a.rounds, 'calls_per_window': a.calls, 'parse': stats(times['parse']), 'k1': stats(times['k1']),
           'bytes_per_pixel': {'parse': 13, 'k1': 24}, 'outputs_agree': same,
           'visible_pixels_by_label': counts[:, :2 + a.blocks, 1].sum(0).tolist(), 'amodal_pixels_by_label': counts[:, :2 + a.blocks, 0].sum(0).tolist()}
    out['ratio_parse_over_k1'] = round(out['parse']['device_ms_median'] / out['k1']['device_ms_median'], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
