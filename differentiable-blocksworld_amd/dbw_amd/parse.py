"""What the blocks world says is in the picture: the result of DifferentiableBlocksWorld.parse_views (ops.parse_scene, csrc/scene_parse.hip)
with the questions a user asks of it.  Plain torch on the four tensors, off the hot path; works on the CPU as on the GPU.

Labels: 0 sky, 1 ground, 2 + k block k in its ORIGINAL index (a block the scene left out keeps its label unused), 255 no face at all."""
import torch

LABEL_SKY, LABEL_GROUND, LABEL_BLOCK0, NO_LABEL, MAX_LABELS = 0, 1, 2, 255, 64
MAX_BLOCKS = MAX_LABELS - LABEL_BLOCK0
GREY_SKY, GREY_GROUND = 0.85, 0.55


def default_palette(block_colors):
    """(256,3) colour of every label value: the env in two greys, block k in block_colors[k], white where there is no face."""
    pal = torch.ones(256, 3)
    pal[LABEL_SKY], pal[LABEL_GROUND] = GREY_SKY, GREY_GROUND
    block_colors = torch.as_tensor(block_colors, dtype=torch.float32).reshape(-1, 3)
    pal[LABEL_BLOCK0:LABEL_BLOCK0 + len(block_colors)] = block_colors
    return pal


class SceneParse:
    """label (N,H,W) uint8, depth (N,H,W) fp32, cover (N,H,W) int64, counts (N,64,2) int32 as ops.parse_scene returns them; n_blocks: blocks
    of the model; kept: (n_blocks,) bool, the blocks the parsed scene contained; palette: (256,3) colours of colors()."""

    def __init__(self, label, depth, cover, counts, n_blocks, kept=None, palette=None):
        if not 0 <= n_blocks <= MAX_BLOCKS:
            raise ValueError(f'{n_blocks} blocks: labels 2 + k must stay below {MAX_LABELS}')
        self.label, self.depth, self.cover, self.counts, self.n_blocks = label, depth, cover, counts, int(n_blocks)
        self.kept = torch.ones(n_blocks, dtype=torch.bool) if kept is None else torch.as_tensor(kept, dtype=torch.bool).cpu()
        self.palette = palette

    def _block_label(self, k):
        if not 0 <= k < self.n_blocks:
            raise IndexError(f'block {k} of {self.n_blocks}')
        return LABEL_BLOCK0 + k

    def amodal(self, k):
        """(N,H,W) bool: block k covers the pixel, seen or hidden.  (>> on int64 is arithmetic: bit 63 arrives at bit 0 like any other.)"""
        return ((self.cover >> self._block_label(k)) & 1).bool()

    def modal(self, k):
        """(N,H,W) bool: block k is what the pixel shows."""
        return self.label == self._block_label(k)

    def foreground(self):
        """(N,H,W) bool: some block is what the pixel shows."""
        return (self.label >= LABEL_BLOCK0) & (self.label != NO_LABEL)

    def areas(self):
        """-> amodal, visible: (N, n_blocks) int64 pixel counts."""
        c = self.counts[:, LABEL_BLOCK0:LABEL_BLOCK0 + self.n_blocks].long()
        return c[..., 0], c[..., 1]

    def occlusion(self):
        """(N, n_blocks) float64: 1 - visible / amodal, NaN where the block covers no pixel of the view."""
        amodal, visible = self.areas()
        amodal, visible = amodal.double(), visible.double()
        return torch.where(amodal > 0, 1 - visible / amodal.clamp(min=1), torch.full_like(amodal, float('nan')))

    def colors(self, palette=None):
        """(N,3,H,W) float: the label map painted -- block k in its colour of get_scene_face_colors, sky and ground in grey, white where no
        face is.  palette: (256,3), or (L,3) for the labels below L."""
        pal = self.palette if palette is None else torch.as_tensor(palette, dtype=torch.float32)
        if pal is None:
            raise ValueError('this SceneParse has no palette: pass one')
        if pal.shape[0] < 256:
            pal = torch.cat([pal, torch.ones(256 - pal.shape[0], 3, dtype=pal.dtype, device=pal.device)], 0)
        return pal.to(self.label.device)[self.label.long()].permute(0, 3, 1, 2).contiguous()
