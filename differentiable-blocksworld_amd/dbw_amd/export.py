"""File writers of the qualitative evaluation (the reference's utils/image.py convert_to_img / save_gif / save_video, utils/mesh.py
save_mesh_as_obj, utils/plot.py-style point clouds): PNG, GIF / mp4, PLY and textured OBJ, with PIL, numpy and the standard library
only.  Frames arrive as 8-bit (H,W,3) arrays -- ops.frames_u8 / renderer.render_views_u8 make them on the GPU -- so nothing here
touches a float image on the hot path.  The OBJ / MTL files are written from the published format (Wavefront OBJ: `v`, `vt`, `f v/vt`,
`mtllib`, `usemtl`; MTL: `newmtl`, `map_Kd`), not from any library's writer."""
import math
import os

import numpy as np
import torch
from PIL import Image

from .structures import Meshes, PackedScene


def _as_u8_hwc(img):
    """(H,W,3) uint8 numpy array out of: the same as array or tensor (host or device); or a float image (3,H,W) / (1,3,H,W) in [0, 1],
    quantised as the reference's convert_to_img does (clamp, times 255, truncate) -- on the GPU by dbw_frames_u8 when it lives there."""
    if torch.is_tensor(img):
        if img.dtype != torch.uint8:
            img = img.detach().float()
            img = img[None] if img.dim() == 3 else img
            if img.dim() != 4 or img.shape[0] != 1 or img.shape[1] != 3:
                raise ValueError(f'a float image is (3,H,W) or (1,3,H,W), got {tuple(img.shape)}')
            if img.is_cuda:
                from . import ops
                img = ops.frames_u8(img)[0]
            else:
                img = (torch.nan_to_num(img[0], nan=0.0).clamp(0, 1) * 255.0).to(torch.uint8).permute(1, 2, 0)
        img = img.detach().cpu().numpy()
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f'an 8-bit image is (H,W,3) uint8, got {img.dtype} {img.shape}')
    return img


def save_png(img, path):
    """One image -> `path` (PNG, lossless).  -> path."""
    Image.fromarray(_as_u8_hwc(img)).save(str(path), format='PNG')
    return str(path)


def save_gif(frames_u8, path, fps=24):
    """(N,H,W,3) uint8 frames -> an animated GIF, every frame on its own adaptive palette (a shared web palette looks very bad: the
    reference's save_gif says so, utils/image.py:66,74), `duration` = 1000 / fps milliseconds per frame, looping."""
    frames = frames_u8.cpu().numpy() if torch.is_tensor(frames_u8) else np.asarray(frames_u8)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or len(frames) == 0:
        raise ValueError(f'frames are (N,H,W,3) uint8 with N > 0, got {frames.dtype} {frames.shape}')
    imgs = [Image.fromarray(np.ascontiguousarray(f)).convert('P', palette=Image.Palette.ADAPTIVE) for f in frames]
    imgs[0].save(str(path), format='GIF', save_all=True, append_images=imgs[1:], duration=int(round(1000 / fps)), loop=0, optimize=False)
    return str(path)


def save_video(frames_u8, path, fps=24):
    """(N,H,W,3) uint8 frames -> a video.  mp4 through imageio's ffmpeg writer where that package imports (the reference's save_video,
    utils/image.py:90-105); otherwise an animated GIF with the same stem.  -> the path written."""
    path = str(path)
    try:
        import imageio
    except ImportError:
        imageio = None
    if imageio is not None:
        frames = frames_u8.cpu().numpy() if torch.is_tensor(frames_u8) else np.asarray(frames_u8)
        imageio.mimwrite(path, frames, format='FFMPEG', fps=fps, quality=10, ffmpeg_log_level='error')
        return path
    return save_gif(frames_u8, os.path.splitext(path)[0] + '.gif', fps=fps)


def join_parses(parses):
    """Several parse.SceneParse of the same model (one per batch of views) -> one over all their views, on the CPU."""
    from .parse import SceneParse
    parses = list(parses)
    if not parses:
        raise ValueError('no parse to join')
    first = parses[0]
    label, depth, cover, counts = [torch.cat([getattr(p, name).cpu() for p in parses], 0) for name in ('label', 'depth', 'cover', 'counts')]
    return SceneParse(label, depth, cover, counts, first.n_blocks, first.kept, first.palette)


def write_parse(parse, path):
    """A parse.SceneParse -> the directory `path`: per view v label_%03d.png (the label map painted: parse.colors()), depth_%03d.npy
    (H,W) float32 and cover_%03d.npy (H,W) int64; and block_visibility.tsv, a line of names and one line per block: `block`, `kept`, then
    per view `amodal_v`, `visible_v` (pixels) and `occlusion_v` (1 - visible / amodal as '{:.5f}', 'nan' for a block the view does not
    contain).  -> the list of the paths written."""
    os.makedirs(str(path), exist_ok=True)
    written = []
    painted = parse.colors().cpu()
    depth, cover = parse.depth.cpu().numpy(), parse.cover.cpu().numpy()
    V = painted.shape[0]
    for v in range(V):
        written.append(save_png(painted[v], os.path.join(str(path), 'label_%03d.png' % v)))
        for name, arr in (('depth', depth), ('cover', cover)):
            written.append(os.path.join(str(path), '%s_%03d.npy' % (name, v)))
            np.save(written[-1], arr[v])
    amodal, visible = [t.cpu() for t in parse.areas()]
    occ = parse.occlusion().cpu()
    written.append(os.path.join(str(path), 'block_visibility.tsv'))
    with open(written[-1], mode='w') as f:
        f.write('\t'.join(['block', 'kept'] + [f'{name}_{v}' for v in range(V) for name in ('amodal', 'visible', 'occlusion')]) + '\n')
        for k in range(parse.n_blocks):
            cells = [str(k), str(int(parse.kept[k]))]
            for v in range(V):
                cells += [str(int(amodal[v, k])), str(int(visible[v, k])), '{:.5f}'.format(float(occ[v, k]))]
            f.write('\t'.join(cells) + '\n')
    return written


def save_ply(path, points):
    """(n,3) points -> a binary little-endian PLY with float x, y, z (eval3d.read_ply_points reads it back).  -> path."""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    pts = np.ascontiguousarray(pts.reshape(-1, 3), dtype='<f4')
    with open(str(path), 'wb') as fh:
        fh.write(('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n'
                  % len(pts)).encode('ascii'))
        fh.write(pts.tobytes())
    return str(path)


# ---------------------------------------------------------------------------------------------------------------------
# textured OBJ
# ---------------------------------------------------------------------------------------------------------------------
def _shelf_layout(sizes):
    """Texel-aligned placement of (h, w) rectangles on shelves, in order: -> [(row, col)], (H, W) of the atlas (each at least 2)."""
    if not sizes:
        return [], (2, 2)
    width = max(max(w for _, w in sizes), int(math.ceil(math.sqrt(sum(h * w for h, w in sizes)))))
    pos, row, col, shelf_h, used_w = [], 0, 0, 0, 0
    for h, w in sizes:
        if col and col + w > width:
            row, col, shelf_h = row + shelf_h, 0, 0
        pos.append((row, col))
        col, shelf_h, used_w = col + w, max(shelf_h, h), max(used_w, col + w)
    return pos, (max(row + shelf_h, 2), max(used_w, 2))


def build_atlas(scene):
    """One texture out of a PackedScene's maps.  -> atlas (Ha,Wa,3) fp32 CPU, face_uvs (F,3,2) float64 CPU into it.

    The project's sampling convention (csrc/shade_math.h footprint_desc = PyTorch3D's TexturesUV with align_corners=True): a map of h x w
    texels with circular padding (pl, pr) along u is sampled as the padded map of wp = w + pl + pr columns, padded column x holding
    source column (x - pl) mod w; (u, v) addresses the continuous texel position (u * (wp - 1), v * (h - 1)) with v = 0 on the BOTTOM
    row (stored row h - 1), bilinear between neighbouring texels, clamped at the border.  The atlas keeps that convention (it is also the
    OBJ one: vt's origin is the bottom-left corner) with (Ha, Wa) in place of (h, wp).  Every map is materialised WITH its padding
    columns (as the reference materialises them with F.pad(mode='circular'), dbw.py:89-93,339-342; a map stored decimated is expanded to
    its full resolution) at an integer texel offset (row r, column c), and its UVs are remapped affinely,
        u' = (c + u * (wp - 1)) / (Wa - 1),      v' = ((Ha - r - h) + v * (h - 1)) / (Ha - 1),
    so that a sample of the atlas at (u', v') lands on the same texel position, between the same two columns and rows, as a sample of
    the map at (u, v): for (u, v) inside [0, 1] the footprint never leaves the map's rectangle (on its last column / row the weight of
    the neighbour outside is zero)."""
    desc = scene.map_desc.detach().cpu().long()
    maps = scene.maps.detach().float().cpu()
    face_uvs = scene.face_uvs.detach().cpu().double()
    face_map = scene.face_map.detach().cpu().long()
    sizes = [(int(d[1]), int(d[2] + d[3] + d[4])) for d in desc]
    pos, (Ha, Wa) = _shelf_layout(sizes)
    atlas = torch.zeros(Ha, Wa, 3)
    ua, ub, va, vb = [torch.zeros(len(desc), dtype=torch.float64) for _ in range(4)]
    for m, (d, (r, c)) in enumerate(zip(desc, pos)):
        off, h, w, pl, pr, sh = [int(x) for x in d[:6]]
        hs, ws, wp = h >> sh, w >> sh, w + pl + pr
        stored = maps[off:off + hs * ws * 3].view(hs, ws, 3)
        rows = torch.arange(h) >> sh
        cols = ((torch.arange(wp) - pl) % w) >> sh
        atlas[r:r + h, c:c + wp] = stored[rows][:, cols]
        ua[m], ub[m] = (wp - 1) / (Wa - 1), c / (Wa - 1)
        va[m], vb[m] = (h - 1) / (Ha - 1), (Ha - r - h) / (Ha - 1)
    uv = torch.stack([face_uvs[..., 0] * ua[face_map][:, None] + ub[face_map][:, None],
                      face_uvs[..., 1] * va[face_map][:, None] + vb[face_map][:, None]], -1)
    return atlas, uv


def save_scene_as_obj(scene_or_mesh, path):
    """A textured scene (PackedScene, or Meshes with UV textures) -> `path` (.obj), `stem.mtl` and the texture atlas `stem.png` next to it.

    OBJ: one `v x y z` per vertex, one `vt u v` per face corner (3 per face, in face order), `mtllib stem.mtl`, `usemtl mesh`, one
    `f a/b c/d e/f` per face (1-based vertex / texture-coordinate indices).  MTL: material `mesh` with `map_Kd stem.png`.  The atlas and
    the (u, v) written follow the convention build_atlas states: v = 0 is the bottom row of the PNG, texel CENTRES of the first and last
    column / row sit at 0 and 1 (align_corners=True) -- a viewer that puts texel EDGES there shows the same picture shifted by under
    half a texel.  The PNG holds 8-bit texels (truncated, like every image the evaluation writes).  -> path."""
    scene = PackedScene.from_meshes(scene_or_mesh) if isinstance(scene_or_mesh, Meshes) else scene_or_mesh
    path = str(path)
    stem = os.path.splitext(os.path.basename(path))[0]
    folder = os.path.dirname(path)
    atlas, uv = build_atlas(scene)
    save_png(atlas.permute(2, 0, 1), os.path.join(folder, stem + '.png'))
    with open(os.path.join(folder, stem + '.mtl'), 'w') as fh:
        fh.write(f'newmtl mesh\nKa 1.000 1.000 1.000\nKd 1.000 1.000 1.000\nKs 0.000 0.000 0.000\nd 1.0\nillum 1\nmap_Kd {stem}.png\n')
    verts = scene.verts.detach().cpu().double().numpy()
    faces = scene.faces.detach().cpu().long().numpy() + 1
    uv = uv.reshape(-1, 2).numpy()
    lines = [f'mtllib {stem}.mtl', 'o mesh']
    lines += ['v %.9g %.9g %.9g' % tuple(v) for v in verts]
    lines += ['vt %.9f %.9f' % tuple(t) for t in uv]
    lines.append('usemtl mesh')
    lines += ['f %d/%d %d/%d %d/%d' % (f[0], 3 * i + 1, f[1], 3 * i + 2, f[2], 3 * i + 3) for i, f in enumerate(faces)]
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return path


def load_obj_as_scene(path, device='cpu'):
    """The files save_scene_as_obj wrote -> a PackedScene with ONE map (the atlas, no padding): the round trip the tests render."""
    path = str(path)
    folder = os.path.dirname(path)
    verts, vts, faces, fvt, png = [], [], [], [], None
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == 'v':
            verts.append([float(x) for x in tok[1:4]])
        elif tok[0] == 'vt':
            vts.append([float(x) for x in tok[1:3]])
        elif tok[0] == 'f':
            pairs = [t.split('/') for t in tok[1:4]]
            faces.append([int(p[0]) - 1 for p in pairs])
            fvt.append([int(p[1]) - 1 for p in pairs])
        elif tok[0] == 'mtllib':
            for ml in open(os.path.join(folder, tok[1])):
                if ml.split()[:1] == ['map_Kd']:
                    png = os.path.join(folder, ml.split()[1])
    atlas = torch.from_numpy(np.array(Image.open(png).convert('RGB'))).float() / 255
    vts = torch.tensor(vts, dtype=torch.float64)
    face_uvs = vts[torch.tensor(fvt)].float()
    desc, _ = PackedScene.describe_maps([tuple(atlas.shape[:2])], [(0, 0)], device)
    return PackedScene(torch.tensor(verts, dtype=torch.float64).float().to(device), torch.tensor(faces, dtype=torch.int32).to(device),
                       face_uvs.contiguous().to(device), torch.zeros(len(faces), dtype=torch.int32, device=device), desc,
                       atlas.reshape(-1).contiguous().to(device))
