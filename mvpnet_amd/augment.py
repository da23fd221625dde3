"""Device-side counterpart of the loader's geometric augmentation (mvpnet/data/scannet_2d3d.py:293-296 horizontal flip per
view, :400-409 rotation about z), for batches that are lifted on the device (`depth`, `cam_matrix`, `pose` in the data dict
instead of loader-computed `knn_indices` / `image_xyz`).

The random DRAWS stay on the host, as in the reference (numpy RNG: one `rand()` per view for the flip, one `uniform(lo, hi)`
angle per chunk); what they select is applied by the HIP kernels where the reference applies it: the flip changes the flat
pixel ids / feature rows (mvp_lift_aug_f32), the rotation acts on `points` and the gathered `image_xyz` after the k-NN search
(float64 product, one rounding to float32 -- scipy's Rotation.apply).

`color_jitter` (scannet_2d3d.py:241-243, T.ColorJitter on the PIL image) is applied by ops.prepare_frames to the frames picked from a
raw uint8 store; `draw_color_jitter` / `draw_flip` below make its draws ON THE DEVICE (torchvision's law, not its draws), which is how
scene.sample_train_batch builds a jittered, mirrored batch without a host synchronisation.  DeviceAugmentation does not touch colours.

The 3D baselines rotate by another law (mvpnet/data/transforms.py:64-92, `RandomRotateZ`): an angle uniform in RADIANS, a float32 matrix,
applied to `points` as `v @ R.T` in float32 before the network.  `draw_z_rotation` draws those matrices on the device; ops.gather_cloud
applies them (scene.sample_train_batch_3d)."""
import math

import numpy as np
import torch


def z_rotation_matrix(angle_deg):
    """3x3 float64 matrix of scipy.spatial.transform.Rotation.from_euler('z', angle, degrees=True): taken from scipy itself
    when it is installed (the reference's own dependency), otherwise from the same unit-quaternion formula."""
    try:
        from scipy.spatial.transform import Rotation
        return Rotation.from_euler('z', float(angle_deg), degrees=True).as_matrix().astype(np.float64)
    except ImportError:
        half = np.deg2rad(float(angle_deg)) / 2.0
        z, w = np.sin(half), np.cos(half)
        n = np.sqrt(z * z + w * w)
        z, w = z / n, w / n
        z2, w2, zw = z * z, w * w, z * w
        return np.array([[w2 - z2, -2.0 * zw, 0.0], [2.0 * zw, w2 - z2, 0.0], [0.0, 0.0, z2 + w2]], np.float64)


class DeviceAugmentation(object):
    """flip: probability of mirroring each view; z_rot: () or (low, high) degrees.  __call__(batch) adds
      'flip'  (B, nv) uint8 and mirrors the flagged views of batch['images'] (the 2D network must see the mirrored image),
      'z_rot' (B, 3, 3) float64 rotation matrices,
    which MVPNet3D.forward / ops.lift consume.  rng: a numpy RandomState / Generator-like with rand() and uniform()."""

    def __init__(self, flip=0.0, z_rot=(), rng=None):
        self.flip = float(flip)
        self.z_rot = tuple(z_rot) if z_rot else ()
        if self.z_rot and len(self.z_rot) != 2:
            raise ValueError('z_rot must be () or (low, high) in degrees')
        self.rng = np.random if rng is None else rng

    def __call__(self, batch):
        ref = batch['depth'] if 'depth' in batch else batch['images']
        B, nv = int(ref.shape[0]), int(ref.shape[1])
        dev = ref.device
        if self.flip:
            flags = np.array([[self.rng.rand() < self.flip for _ in range(nv)] for _ in range(B)], dtype=bool)
            flip = torch.from_numpy(flags.astype(np.uint8)).to(dev)
            batch['flip'] = flip
            if 'images' in batch and flags.any():
                images = batch['images']                                   # (B, nv, 3, h, w)
                batch['images'] = torch.where(flip.bool().view(B, nv, 1, 1, 1), images.flip(-1), images)
        if self.z_rot:
            mats = np.stack([z_rotation_matrix(self.rng.uniform(low=self.z_rot[0], high=self.z_rot[1])) for _ in range(B)])
            batch['z_rot'] = torch.from_numpy(mats).to(dev)
        return batch


def _shape(n):
    return (int(n),) if isinstance(n, int) else tuple(int(v) for v in n)


def draw_color_jitter(n, params, device, generator=None):
    """The draws of torchvision's ColorJitter(brightness, contrast, saturation) for n frames (an int, or a shape such as (B, nv)), on
    `device` without a host synchronisation.  params: the YAML's `color_jitter` 3-tuple; a fourth entry (hue) must be 0.
    -> factor n + (3,) float32, order n + (3,) uint8 -- what ops.prepare_frames takes.  The law: every factor uniform in
    [max(0, 1 - p), 1 + p], drawn in float64 and rounded once to float32; the order a uniform permutation of the enabled ops (the argsort
    of three uniforms), 0 brightness, 1 contrast, 2 saturation.  A parameter of 0 disables its op: factor exactly 1, order code 3 behind
    the enabled ones.  generator: one of `device`, or None for its global generator."""
    p = tuple(float(v) for v in params)
    if len(p) == 4:
        if p[3] != 0.0:
            raise ValueError('draw_color_jitter: hue jitter is not supported (the reference configs pass three numbers)')
        p = p[:3]
    if len(p) != 3 or min(p) < 0.0:
        raise ValueError('color_jitter must be (brightness, contrast, saturation), each >= 0')
    shape = _shape(n)
    u = torch.rand(shape + (6,), dtype=torch.float64, generator=generator, device=device)
    lo = [max(0.0, 1.0 - v) for v in p]
    factor = torch.stack([u[..., i] * ((1.0 + p[i]) - lo[i]) + lo[i] if p[i] else torch.ones_like(u[..., i]) for i in range(3)], dim=-1).float()
    keys = torch.stack([u[..., 3 + i] if p[i] else u[..., 3 + i] + 2.0 for i in range(3)], dim=-1)  # disabled ops sort behind the others
    order = keys.argsort(dim=-1).to(torch.uint8)
    enabled = sum(1 for v in p if v)
    if enabled < 3:
        order[..., enabled:] = 3
    return factor.contiguous(), order.contiguous()


def draw_flip(n, p, device, generator=None):
    """n (an int or a shape) horizontal-flip flags as uint8 on `device`: 1 with probability p (`np.random.rand() < flip`,
    scannet_2d3d.py:293), drawn on the device."""
    return (torch.rand(_shape(n), dtype=torch.float64, generator=generator, device=device) < float(p)).to(torch.uint8)


def draw_frames(n, Ftot, device, generator=None):
    """n (an int or a shape) frame rows uniform in [0, Ftot) as int64 on `device`, without a host synchronisation: for callers of
    scene.sample_train_batch_2d that have no sampler of their own.  The rows are drawn WITH replacement, every batch on its own; the
    reference shuffles an epoch (a DataLoader with shuffle=True over ScanNet2D: every frame once per epoch, without replacement)."""
    return torch.randint(0, int(Ftot), _shape(n), dtype=torch.int64, generator=generator, device=device)


def z_rotation_from_angle(angle):
    """angle (...,) float64 radians -> (...,3,3) float32 [[c,-s,0],[s,c,0],[0,0,1]]: c and s computed in float64 and rounded once, the
    matrix `Rotation.from_rotvec(angle * (0,0,1)).as_dcm().astype(np.float32)` of transforms.py:73-76 up to that rounding."""
    angle = angle.double()
    c, s = torch.cos(angle), torch.sin(angle)
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    return torch.stack([c, -s, zero, s, c, zero, zero, zero, one], dim=-1).view(angle.shape + (3, 3)).float().contiguous()


def draw_z_rotation(n, low=-math.pi, high=math.pi, device=None, generator=None):
    """n (an int or a shape) rotations about z by `transforms.RandomRotate`'s law (mvpnet/data/transforms.py:68-76; RandomRotateZ's defaults),
    drawn on `device` without a host synchronisation: angle = low + (high - low) * u with u uniform in [0, 1) in float64 (numpy's
    uniform(low, high)), -> n + (3,3) float32 (z_rotation_from_angle).  generator: one of `device`, or None for its global generator."""
    u = torch.rand(_shape(n), dtype=torch.float64, generator=generator, device=device)
    return z_rotation_from_angle(float(low) + (float(high) - float(low)) * u)
