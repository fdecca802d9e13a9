import torch

from ..augment import check_ranges, mesh_affine, random_mesh_affine
from ..norm import whole_ptr
from ..pooling import mesh_mean


class RandomMeshAffine(object):
    """The augmentation of the reference's notebooks -- Compose((Center() | RandomScale(scale), RandomRotate(d0, axis=0),
    RandomRotate(d1, axis=1), RandomRotate(d2, axis=2))) -- for a whole MeshBatch at once, on the device: every mesh gets its own
    centre (the mean of its vertices, center=True), scale (uniform in `scale`, or none) and three rotation angles (uniform in
    [-degrees[k], degrees[k]]), drawn by fieldconv_amd.augment.random_mesh_affine from (seed, step, mesh).

        augment = RandomMeshAffine(scale=(0.85, 1.15))
        x = net(augment.input(batch), ...)              # (S,3): the augmented positions of the sampled vertices only
        batch = augment(batch)                          # or: batch.pos replaced by the augmented positions of every vertex

    __call__(data) takes a MeshBatch or a single mesh (any object with pos (V,3) float32 on a ROCm device: B = 1) and sets data.pos
    to a NEW tensor; the caller's tensor is not written.  logMag, logAng, xp, w and the graph stay as they are: augmentation
    comes after the precomputation, as in the notebooks (a scale does not touch logMag there either).  NormalizeAxes after it is
    the caller's business.  seed=None draws the seed once at construction from torch's default CPU generator (torch.manual_seed
    governs it).  Every call (__call__ or input) draws with the current step and advances it by one; `step` is a (1,) int64 tensor
    on the data's device, read by the kernel itself, so a call costs no synchronisation.  Three launches with center (the segment
    mean's two and the apply), else one, after the draw's one."""

    def __init__(self, scale=None, degrees=(45, 45, 45), center=False, seed=None):
        has_scale, lo, hi, self.degrees = check_ranges(scale, degrees, 'RandomMeshAffine')
        self.scale = (lo, hi) if has_scale else None
        if not isinstance(center, bool):
            raise ValueError(f'RandomMeshAffine: center must be True or False, got {center!r}')
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
        elif isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError(f'RandomMeshAffine: seed must be an integer in [0, 2^64) or None, got {seed!r}')
        self.center, self.seed = center, int(seed)
        self.step = None          # (1,) int64 on the device of the first mesh seen

    def _draw(self, data, index):
        pos = data.pos
        if not torch.is_tensor(pos) or pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype != torch.float32:
            raise ValueError('RandomMeshAffine: data.pos must be a (V,3) float32 tensor, got '
                             f'{(tuple(pos.shape), pos.dtype) if torch.is_tensor(pos) else type(pos).__name__}')
        if not pos.is_cuda:
            raise RuntimeError(f'RandomMeshAffine: data.pos is on {pos.device}; fieldconv_amd augmentation runs on a ROCm device and has no CPU path')
        pos_ptr = getattr(data, 'pos_ptr', None)
        if pos_ptr is None:
            pos_ptr = whole_ptr(int(pos.shape[0]), pos.device)
        if self.step is None or self.step.device != pos.device:
            self.step = torch.zeros(1, dtype=torch.int64, device=pos.device) if self.step is None else self.step.to(pos.device)
        B = int(pos_ptr.numel()) - 1
        t = mesh_mean(pos, pos_ptr) if self.center else None
        _, M = random_mesh_affine(B, self.seed, self.step, self.scale, self.degrees)
        out = mesh_affine(pos, pos_ptr, M, t, index)
        self.step.add_(1)
        return out

    def __call__(self, data):
        data.pos = self._draw(data, None)
        return data

    def input(self, data):
        """(S,3): the augmented positions of the sampled vertices, pos'[data.sample_idx], without forming pos'"""
        index = getattr(data, 'sample_idx', None)
        if index is None:
            raise ValueError('RandomMeshAffine.input: data has no sample_idx (run SupportGraph first, or call the transform itself)')
        return self._draw(data, index)

    def __repr__(self):
        return '{}(scale={}, degrees={}, center={}, seed={})'.format(self.__class__.__name__, self.scale, self.degrees, self.center, self.seed)
