"""Records the two MeshEvaluator cases of tests/icp_fixture.py: their inputs (the ground truth and the samples, drawn here once: which face
a sample falls on depends on the last bit of the face areas, so another processor may draw other points from the same seed) and their
scores by the CPU path (eval3d.gradient_icp_torch, chamfer_distance on torch brute-force searches) in fp32 and in fp64.  The GPU tests hold
the device to the fp64 scores with a bar made of the difference between the two.  Run from the repository root:

    python tests/golden/make_icp_golden.py sphere
        tests/golden/icp_sphere_inputs.npz, icp_sphere_scores.json (with a checksum of the samples): sphere_case()
    python tests/golden/make_icp_golden.py dump-blocks FILE
        needs a GPU (the model builds its blocks there only): writes the live blocks of blocks_model() to FILE (.npz: verts, faces)
    python tests/golden/make_icp_golden.py blocks FILE
        tests/golden/icp_blocks_inputs.npz, icp_blocks_scores.json from that FILE: blocks_case(), both clouds in the ground truth's
        unit-cube frame as evaluate_aligned makes it"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
from dbw_amd import eval3d                                      # noqa: E402
import icp_fixture as fx                                        # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else ''
if mode == 'sphere':
    np.savez_compressed(fx.SPHERE_INPUTS, **fx.draw_sphere_inputs())
    (verts, faces), pc_gt, norm_gt, ev, samples = fx.sphere_case()
    out = {'fp32': dict(ev.evaluate((verts, faces), pc_gt, norm_gt, samples=samples)),
           'fp64': dict(ev.evaluate((verts.double(), faces), pc_gt, norm_gt, samples=samples)),
           'checksum': fx.sphere_checksum()}
    with open(fx.SPHERE_GOLDEN, 'w') as f:
        json.dump(out, f, indent=1)
    print(out)
elif mode == 'dump-blocks':
    verts, faces = fx.blocks_model('cuda').blocks_mesh(filter_transparent=True)
    np.savez(sys.argv[2], verts=verts.detach().cpu().numpy(), faces=faces.cpu().numpy())
    print(tuple(verts.shape), tuple(faces.shape))
elif mode == 'blocks':
    with np.load(sys.argv[2]) as z:
        verts, faces = torch.from_numpy(z['verts']), torch.from_numpy(z['faces'])
    np.savez_compressed(fx.BLOCKS_INPUTS, **fx.draw_blocks_inputs(verts, faces))
    verts_unit, gt, gt_n, samples = fx.blocks_case()
    off, sc = eval3d.unit_cube_frame(gt)
    ev = fx.blocks_evaluator()
    out = {'fp32': dict(ev.evaluate((verts_unit, faces), (gt - off) / sc, gt_n, samples=samples)),
           'fp64': dict(ev.evaluate((verts_unit.double(), faces), (gt - off) / sc, gt_n, samples=samples))}
    with open(fx.BLOCKS_GOLDEN, 'w') as f:
        json.dump(out, f, indent=1)
    print(out)
else:
    sys.exit(__doc__)
