"""The 3D baselines' batch on the device (new: the reference runs `CropPad` / `RandomRotateZ` per sample in a data-loader worker,
mvpnet/data/transforms.py:64-133 behind mvpnet/data/scannet_3d.py:135-221): the crop / pad of whole scenes and the gather that turns a
`choice` into PN2SSG's inputs."""
import torch

from .. import _lib as L
from .sample import MAX_CHUNKS, _i64, _seed, _workspace

MAX_SCENE_NB_PTS = L.LIMITS['MVP_SAMPLE_SCENE_MAX_PTS']  # what the sampler's multi-workgroup FPS serves


def _scenes(scene_offsets, scene_of_row, who):
    if _i64(scene_offsets, 'scene_offsets', who).dim() != 1 or scene_offsets.numel() < 2:
        raise RuntimeError(who + ': scene_offsets must be (S+1,), S >= 1')
    if _i64(scene_of_row, 'scene_of_row', who).dim() != 1:
        raise RuntimeError(who + ': scene_of_row must be (B,)')
    return scene_offsets.numel() - 1, scene_of_row.numel()


def sample_scenes(scene_offsets, scene_of_row, nb_pts, seed=0, Ntot=None):
    """`CropPad(nb_pts)` of B whole scenes in one call, no host synchronisation.  scene_offsets (S+1,) int64 and scene_of_row (B,) int64 on
    the device; seed: an int, or an int64 tensor of one element on the device (a captured graph then draws afresh on every replay).
    Ntot: the points of the store (`points.size(0)`, a host number) where the caller has it: the offsets are cut to it and the passes'
    grids are sized by it; None: the limit of 2^31 - 1 stands in (nothing here reads a tensor back, and the draw reads no array of that
    length; the choice is the same either way).  -> dict: choice (B,nb_pts) int64 inside the scene, num_points (B,) int32.
    Definition (pinned): include/mvp_hip.h, mvp_sample_scenes_f32."""
    L.require_gpu(scene_offsets, scene_of_row)
    S, B = _scenes(scene_offsets, scene_of_row, 'sample_scenes')
    Ntot, nb_pts = 2 ** 31 - 1 if Ntot is None else int(Ntot), int(nb_pts)
    if not (1 <= nb_pts <= MAX_SCENE_NB_PTS and B <= MAX_CHUNKS and 1 <= Ntot < 2 ** 31):
        raise RuntimeError('sample_scenes: needs 1 <= nb_pts <= {}, B <= {} and 1 <= Ntot < 2^31'.format(MAX_SCENE_NB_PTS, MAX_CHUNKS))
    seed, seed_dev = _seed(seed, 'sample_scenes')
    dev = scene_offsets.device
    out = {'choice': torch.empty((B, nb_pts), dtype=torch.int64, device=dev), 'num_points': torch.empty((B,), dtype=torch.int32, device=dev)}
    if B == 0:
        return out
    ws, nbytes = _workspace('mvp_sample_scenes', dev, Ntot, B, nb_pts)
    L.call('mvp_sample_scenes_f32', scene_offsets, L.ptr(scene_offsets), L.ptr(scene_of_row), Ntot, S, B, nb_pts, seed, L.ptr(seed_dev),
           L.ptr(out['choice']), L.ptr(out['num_points']), L.ptr(ws), nbytes)
    return out


def gather_cloud(points, scene_offsets, scene_of_row, choice, seg_label=None, colors=None, rot=None):
    """A `choice` of ops.sample_scenes or ops.sample_chunks as the network's inputs, one launch.  points (Ntot,3) float32, seg_label (Ntot,)
    int64 or None, colors (Ntot,3) uint8 or None: the store; scene_offsets (S+1,), scene_of_row (B,), choice (B,nb_pts) int64; rot (B,3,3)
    float32 or None.  -> dict: points (B,3,nb_pts) float32 = `points[choice] @ R.T` in float32 (rot None: an exact copy)
    [, seg_label (B,nb_pts) int64] [, feature (B,3,nb_pts) float32 = colors / 255].  Definition: include/mvp_hip.h, mvp_gather_cloud_f32."""
    L.require_gpu(points, seg_label, colors, scene_offsets, scene_of_row, choice, rot)
    who = 'gather_cloud'
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32 or points.size(0) < 1 or not points.is_contiguous():
        raise RuntimeError('gather_cloud: points must be contiguous (Ntot,3) float32, Ntot >= 1')
    Ntot = points.size(0)
    S, B = _scenes(scene_offsets, scene_of_row, who)
    if _i64(choice, 'choice', who).dim() != 2 or choice.size(0) != B or choice.size(1) < 1 or not choice.is_contiguous():
        raise RuntimeError('gather_cloud: choice must be contiguous (B,nb_pts), nb_pts >= 1')
    nb_pts = choice.size(1)
    if seg_label is not None and (_i64(seg_label, 'seg_label', who).shape != (Ntot,) or not seg_label.is_contiguous()):
        raise RuntimeError('gather_cloud: seg_label must be (Ntot,)')
    if colors is not None and (colors.dtype != torch.uint8 or colors.shape != (Ntot, 3) or not colors.is_contiguous()):
        raise RuntimeError('gather_cloud: colors must be contiguous (Ntot,3) uint8')
    if rot is not None and (rot.dtype != torch.float32 or rot.shape != (B, 3, 3) or not rot.is_contiguous()):
        raise RuntimeError('gather_cloud: rot must be contiguous (B,3,3) float32')
    if B > MAX_CHUNKS or nb_pts >= 2 ** 31:
        raise RuntimeError('gather_cloud: needs B <= {} and nb_pts < 2^31'.format(MAX_CHUNKS))
    dev = points.device
    out = {'points': torch.empty((B, 3, nb_pts), dtype=torch.float32, device=dev)}
    if seg_label is not None:
        out['seg_label'] = torch.empty((B, nb_pts), dtype=torch.int64, device=dev)
    if colors is not None:
        out['feature'] = torch.empty((B, 3, nb_pts), dtype=torch.float32, device=dev)
    if B == 0:
        return out
    L.call('mvp_gather_cloud_f32', points, L.ptr(points), L.ptr(seg_label), L.ptr(colors), L.ptr(scene_offsets), L.ptr(scene_of_row), L.ptr(choice),
           L.ptr(rot), Ntot, S, B, nb_pts, L.ptr(out['points']), L.ptr(out.get('seg_label')), L.ptr(out.get('feature')))
    return out
