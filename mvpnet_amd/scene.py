"""Whole-scene inference: the loop of mvpnet/test_mvpnet_3d.py:142-174 re-organised for one process per GPU.

The reference feeds the chunks of a scene ONE at a time through the network on one GPU and accumulates
`pred_logit_whole_scene[chunk_ind] += logit`, `num_pred_per_point[chunk_ind] += 1` on the host.  Here rank r takes chunks
r, r+W, ... (dist.shard_chunks), runs them in batches with the coordinate-only work of the next batch prefetched on the side
stream, the per-chunk logits are all-gathered ONCE (RCCL over xGMI) and every rank votes on the device (dist.vote_scene)."""
import torch

from . import chunks as CH
from . import dist as D
from . import metric
from . import ops
from .mvpnet3d import prefetch_geometry
from .nn import eval_mode


def _unwrap(model):
    return model.module if hasattr(model, 'module') else model


def _check_scene_points(who, points):
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32 or not points.is_cuda:
        raise RuntimeError(who + ': points must be (n,3) float32 on the device')


def _no_prediction(n_pts, num_classes, dev):
    """What every whole-scene path returns for a scene without a kept window: zero logits, labels all `num_classes`, zero counts."""
    return (torch.zeros((n_pts, num_classes), dtype=torch.float32, device=dev), torch.full((n_pts,), num_classes, dtype=torch.int64, device=dev),
            torch.zeros((n_pts,), dtype=torch.int32, device=dev))


def pad_sparse_chunk(data, min_nb_pts=2048, generator=None):
    """The reference's rule for chunks with fewer than `min_nb_pts` points (test_mvpnet_3d.py:146-154; FPS needs at least
    as many points as centroids): append randomly chosen duplicates of the chunk's own points.  `data`: one chunk's dict with
    'points' (3, n) [+ 'knn_indices' (n, k)] as tensors; returns a dict whose arrays have max(n, min_nb_pts) points.  The
    logits of the appended points are dropped by the vote (only the first len(chunk_ind) columns are used)."""
    n = data['points'].size(1)
    if n >= min_nb_pts:
        return data
    choice = CH.crop_pad_choice(n, min_nb_pts, generator=generator, device='cpu').to(data['points'].device)  # drawn on the host
    out = dict(data, points=data['points'][:, choice])
    if 'knn_indices' in data:
        out['knn_indices'] = data['knn_indices'][choice]
    return out


def infer_scene(model, chunk_batches, chunk_inds, n_pts, num_chunks=None, num_classes=None):
    """model: MVPNet3D / PN2SSG on this rank's GPU; run in eval mode under no_grad, its mode is restored (also when a forward raises).
    chunk_batches: list of data dicts (the reference's keys, tensors on the device) holding THIS RANK's chunks in the order
        `dist.shard_chunks(num_chunks, rank, world)`, any batch sizes.  Chunks may have DIFFERENT numbers of points (the
        reference feeds every chunk with all its points, `nb_pts=-1`, padded to >= 2048: pad_sparse_chunk): every batch holds
        chunks of one size (a ragged scene is simply passed as batches of 1, or grouped by size: prepare_scene_bucketed pads
        chunks of similar size to a common one); a rank may hold none.
    chunk_inds: list over ALL chunks (global order) of int64 tensors on the device: scene point ids of each chunk's points;
        `len(chunk_inds[i]) <= N_i`, logits beyond it belong to padded points and are ignored (test_mvpnet_3d.py:160-164).
    n_pts: number of scene points.
    Returns mean logits (n_pts, C), labels (n_pts,) with C = "no prediction" where a point is in no chunk, vote counts."""
    num_chunks = len(chunk_inds) if num_chunks is None else num_chunks
    if num_classes is None:
        net = _unwrap(model)
        num_classes = int(getattr(net, 'net_3d', net).num_classes)
    with eval_mode(model):
        outs = _forward_batches(model, chunk_batches)
    return _vote_chunk_logits(outs, chunk_inds, n_pts, num_chunks, num_classes)


def _forward_batches(model, chunk_batches, ready=None):
    """infer_scene's loop: the batches through `model` (in eval mode already) under no_grad, the coordinate-only work planned ahead on the
    side stream -> the batches' seg_logit.  ready(i, batch) -> the dict batch i is fed as, called right before its forward (infer_scene_shared
    hangs the run's feature store in there); the planning reads `points` only, so it never waits for it."""
    ready = ready or (lambda i, b: b)
    outs = []
    net = _unwrap(model)
    net3d = getattr(net, 'net_3d', net)
    clouds = sum(b['points'].size(0) for b in chunk_batches)
    same_n = len({b['points'].size(2) for b in chunk_batches}) <= 1
    with torch.no_grad():
        if len(chunk_batches) > 1 and same_n and clouds <= 256 and hasattr(net3d, 'plan_geometry') and chunk_batches[0]['points'].is_cuda \
                and all('geometry_plan' not in b for b in chunk_batches):
            # Farthest point sampling occupies ONE CU per cloud for ~2.8 ms whatever the batch size (256 CUs): the coordinate-only
            # work of ALL this rank's chunks is planned in one call on the side stream and sliced per batch.
            pts = torch.cat([b['points'] for b in chunk_batches]).transpose(1, 2).contiguous()
            side = net._side_stream(pts.device) if hasattr(net, '_side_stream') else torch.cuda.Stream(device=pts.device)
            plan = net3d.plan_geometry(pts, stream=side, with_csr=False)
            lo = 0
            for i, b in enumerate(chunk_batches):
                hi = lo + b['points'].size(0)
                outs.append(model(dict(ready(i, b), geometry_plan=net3d.slice_plan(plan, lo, hi)))['seg_logit'])
                lo = hi
        else:
            cur = prefetch_geometry(model, dict(chunk_batches[0])) if chunk_batches else None
            for i in range(len(chunk_batches)):
                nxt = dict(chunk_batches[i + 1]) if i + 1 < len(chunk_batches) else None
                cur = ready(i, cur)
                outs.append(model(cur if nxt is None else dict(cur, prefetch_next=nxt))['seg_logit'])
                cur = nxt
    return outs


def _vote_chunk_logits(outs, chunk_inds, n_pts, num_chunks, num_classes):
    """infer_scene's tail: the batches' logits brought to one width, gathered over the ranks and voted into the scene."""
    # One common column count for the collective: the largest VALID length of any chunk of the scene -- known on every rank
    # from the (host-known) index lists, so no shape exchange is needed.  Columns beyond a chunk's own valid length are
    # never read by the vote, so cutting a longer (padded) chunk there loses nothing.
    width = max((int(ind.numel()) for ind in chunk_inds), default=1)
    if outs and all(o.size(2) == width for o in outs):
        local = torch.cat(outs)
    else:
        dev = chunk_inds[0].device if chunk_inds else (outs[0].device if outs else torch.device('cpu'))
        local = torch.zeros((sum(o.size(0) for o in outs), num_classes, width), dtype=torch.float32, device=dev)
        lo = 0
        for o in outs:
            n = min(width, o.size(2))
            local[lo:lo + o.size(0), :, :n] = o[:, :, :n]
            lo += o.size(0)
    logits = D.all_gather_logits(local, num_chunks)
    return D.vote_scene(logits, chunk_inds, n_pts)


def infer_scene_votes(model, points, feature=None, nb_pts=32768, num_votes=3, vote_inds=None, generator=None):
    """The whole-scene test path of the 3D baseline (mvpnet/test_3d_scene.py:127-164, configs/scannet/3d_baselines/pn2ssg_scene.yaml):
    `num_votes` random subsamples of the scene go through `model` as ONE batch, every subsample's logits are propagated to all scene
    points through each point's nearest sampled point, and the votes are averaged.  Single process.
    model: PN2SSG (anything that maps {'points' (V,3,nb), ['feature' (V,3,nb)]} to {'seg_logit' (V,C,nb)}) on the points' GPU.
    points (n,3) float32 on the device; feature (n,3) float32 or None: the colours, for a model with in_channels = 3.
    vote_inds (V,nb_pts) int64 in [0, n): the subsamples, instead of the draw -- nb_pts, num_votes and generator are then NOT used, the
    tensor's shape decides -- (the reference's np.random.choice draws can be replayed exactly);
    otherwise per vote, as :128-131, `torch.randperm(n, generator=generator)[:nb_pts]` when n >= nb_pts -- the generator's device
    decides where the permutation is drawn --, else arange(n) followed by nb_pts - n times index 0 (the reference's np.zeros padding).
    -> mean logits (n,C), labels (n,) -- every point gets one, this path has no "no prediction" class --, vote_inds (V,nb_pts).
    The propagation is ops.vote_nearest (nearest by float32 distance, lowest index on ties, votes added in order), the division by the
    number of votes and the argmax are mvp_vote_finish_f32."""
    dev = points.device
    n = points.size(0)
    if points.dim() != 2 or points.size(1) != 3 or n < 1:
        raise RuntimeError('infer_scene_votes: points must be (n,3), n >= 1')
    if feature is not None and (feature.dim() != 2 or feature.size(0) != n):
        raise RuntimeError('infer_scene_votes: feature must be (n,channels)')
    if vote_inds is None:
        if not (1 <= num_votes < 65536 and 1 <= nb_pts <= ops.vote.MAX_KEYS):
            raise RuntimeError('infer_scene_votes: needs 1 <= num_votes < 65536 and 1 <= nb_pts <= {}'.format(ops.vote.MAX_KEYS))
        picks = []
        for _ in range(int(num_votes)):
            if n >= nb_pts:
                gdev = generator.device if generator is not None else dev
                picks.append(torch.randperm(n, generator=generator, device=gdev)[:nb_pts].to(dev))
            else:
                picks.append(torch.cat([torch.arange(n, device=dev), torch.zeros(nb_pts - n, dtype=torch.int64, device=dev)]))
        vote_inds = torch.stack(picks)
    else:
        # checked before the forward pass, not after it (the range check reads two numbers back from the device)
        vote_inds = torch.as_tensor(vote_inds).to(dev).long()
        if vote_inds.dim() != 2 or not (1 <= vote_inds.size(0) < 65536 and 1 <= vote_inds.size(1) <= ops.vote.MAX_KEYS):
            raise RuntimeError('infer_scene_votes: vote_inds must be (V,nb_pts) with 1 <= V < 65536 and 1 <= nb_pts <= {}'.format(ops.vote.MAX_KEYS))
        if int(vote_inds.min()) < 0 or int(vote_inds.max()) >= n:
            raise RuntimeError('infer_scene_votes: vote_inds must lie in [0, {})'.format(n))
    V = vote_inds.size(0)
    keys = points[vote_inds]  # (V,nb,3)
    batch = {'points': keys.transpose(1, 2).contiguous()}
    if feature is not None:
        batch['feature'] = feature[vote_inds].transpose(1, 2).contiguous()
    with eval_mode(model):
        logit = model(batch)['seg_logit']  # (V,C,nb), PN2SSG: a transposed view of row-major rows
    total = ops.vote_nearest(points.contiguous(), keys, logit)
    return (*ops.vote_finish(total, torch.full((n,), V, dtype=torch.int32, device=dev)), vote_inds)


def prepare_scene(points, depth, cam_matrix, pose, images, *, chunk_size, chunk_stride, chunk_thresh, chunk_margin, num_rgbd_frames, k,
                  min_nb_pts=2048, overlap=None, batch_size=8, lift_depth=None, num_base_pts=2000, radius=0.1, generator=None,
                  pad_generator=None, image_normalizer=None, channels_last=False):
    """From a scene's raw arrays to what `infer_scene` takes: `ScanNet2D3DChunksTest.__getitem__` (mvpnet/data/scannet_2d3d.py:506-565)
    followed by `get_rgbd_data`'s frame choice (:191-221) and the sparse-chunk rule of test_mvpnet_3d.py:146-154, on the device.

    points (n,3) float32; depth (F,h,w) float32 m / (u)int16 mm with intrinsics cam_matrix ((3,3) or (4,4), of depth's resolution);
    pose (F,4,4) float32; images (F,3,H,W) what the 2D network reads, or the raw (F,H,W,3) uint8 frames: the picked ones then go through
    ops.prepare_frames (`/ 255.` and `image_normalizer` = the YAML's (mean, std), scannet_2d3d.py:245-251; channels_last: the layout a
    channels-last 2D network reads; no jitter at test time).  The overlap is computed from `depth` as given (the reference
    uses 80x60 maps: chunks.compute_rgbd_overlap); the batches carry the lifting-resolution maps: `lift_depth` (F,H,W), or `depth`
    itself when it already has the images' resolution, with the intrinsics' first two rows scaled by W/w and H/h (:206-210).
    overlap=(base_point_ind, overlaps) -- the reference's per-scene arrays -- skips the overlap computation.

    The result lists ALL chunks of the scene, i.e. what a single process hands to infer_scene; with several ranks every rank passes
    infer_scene the batches of its own shard (dist.shard_chunks) and the full chunk_inds.  Beyond the reference's arguments:
    `lift_depth`, `num_base_pts` / `radius` / `generator` (handed to chunks.compute_rgbd_overlap) and `pad_generator` (pad_sparse_chunk).
    The chunks and their base-point bit rows come from chunks.scene2chunks_csr (the chunker kernels; no membership matrices), all chunks'
    frames from ONE ops.select_frames_batched call on bit rows.  The base points are needed before the chunker runs: for a scene in which
    no window is kept, `generator` has been drawn from and `num_base_pts > n` raises before ([], [], n_pts) is returned.  Every chunk is fed
    whole (nb_pts = -1), padded to `min_nb_pts` by pad_sparse_chunk; consecutive chunks of equal size share a batch of up to `batch_size`,
    the chunk order is kept.
    -> (chunk_batches, chunk_inds, n_pts) with the keys MVPNet3D._forward reads: images (B,nv,3,H,W), points (B,3,N), depth (B,nv,H,W),
    cam_matrix / kinv (B,nv,3,3), pose (B,nv,4,4), pixel_box (B,4) = chunk box -/+ 0.1 m (:274-281), k."""
    csr = _scene_chunks(points, depth, cam_matrix, pose, overlap, num_rgbd_frames, chunk_size, chunk_stride, chunk_thresh, chunk_margin,
                        num_base_pts, radius, generator)
    lengths, n_pts = csr['lengths'], points.size(0)
    if not lengths:
        return [], [], n_pts
    batch = _scene_batcher(points.device, depth, cam_matrix, pose, images, lift_depth, 'prepare_scene', k, image_normalizer, channels_last)
    chunk_inds = list(torch.split(csr['index'], lengths))
    singles = [pad_sparse_chunk({'points': points[ind].t().contiguous()}, min_nb_pts=min_nb_pts, generator=pad_generator)['points'] for ind in chunk_inds]
    chunk_batches, lo = [], 0
    while lo < len(singles):
        hi = lo + 1
        while hi < len(singles) and hi - lo < batch_size and singles[hi].size(1) == singles[lo].size(1):
            hi += 1
        chunk_batches.append(batch(csr['picked'][lo:hi], torch.stack(singles[lo:hi]).contiguous(), csr['pixel_box'][lo:hi]))
        lo = hi
    return chunk_batches, chunk_inds, n_pts


def _scene_chunks(points, depth, cam_matrix, pose, overlap, num_rgbd_frames, chunk_size, chunk_stride, chunk_thresh, chunk_margin, num_base_pts,
                  radius, generator):
    """What prepare_scene and prepare_scene_bucketed share: the scene's chunks and their frames, in the chunker's order.
    -> chunks.scene2chunks_csr's dict (called with the overlap's base points) + picked (C,nv) int64: ONE ops.select_frames_batched call on
    bit rows -- the overlap's (given, or chunks.compute_rgbd_overlap's) and the chunker's base_bits -- and pixel_box (C,4) float32."""
    dev = points.device
    if overlap is None:
        base_point_ind, ov = CH.compute_rgbd_overlap(points, depth, cam_matrix, pose, num_base_pts=num_base_pts, radius=radius, generator=generator,
                                                     packed=True)
    else:
        base_point_ind, ov = overlap
        base_point_ind = torch.as_tensor(base_point_ind).to(dev).long()
        ov = torch.as_tensor(ov).to(dev)
        ov = ov if ov.dtype == torch.int32 else ops.pack_bits(ov.bool().t())
    csr = CH.scene2chunks_csr(points, chunk_size, chunk_stride, thresh=chunk_thresh, margin=chunk_margin, base_point_ind=base_point_ind.contiguous())
    if csr['lengths']:
        csr['picked'] = ops.select_frames_batched(ov, csr['base_bits'], num_rgbd_frames)
        csr['pixel_box'] = (csr['boxes'][:, [0, 1, 3, 4]] + torch.tensor([-0.1, -0.1, 0.1, 0.1], dtype=torch.float64, device=dev)).float()
    return csr


def _scene_batcher(dev, depth, cam_matrix, pose, images, lift_depth, who, k, image_normalizer=None, channels_last=False):
    """-> batch(sel, points, pixel_box): one batch of a scene, the frames `sel` (B,nv) beside the chunks' points (B,3,N) and pixel boxes (B,4).
    _scene_geometry's batch with `images` (B,nv,3,H,W) as the 2D network reads them."""
    _, geometry = _scene_geometry(dev, depth, cam_matrix, pose, images, lift_depth, who, k, image_normalizer, channels_last)
    return lambda sel, points, pixel_box: dict(geometry(sel, points, pixel_box), images=_test_frames(images, sel, image_normalizer, channels_last))


def _test_frames(images, sel, image_normalizer, channels_last):
    """The frames `sel` (any shape, int64 on the device) as the 2D network reads them at test time: raw (F,H,W,3) uint8 frames through
    ops.prepare_frames, float images -- final, the caller has asked _raw_frames -- by a plain gather."""
    if images.dtype == torch.uint8:
        return ops.prepare_frames(images, sel.contiguous(), normalizer=image_normalizer, channels_last=channels_last)
    return images[sel].contiguous()


def _scene_geometry(dev, depth, cam_matrix, pose, images, lift_depth, who, k, image_normalizer=None, channels_last=False):
    """-> (the lifting-resolution depth maps (F,H,W); geometry(sel, points, pixel_box): one batch of a scene without its images -- depth,
    pose, cam_matrix and kinv of the frames `sel` (B,nv) beside points, pixel_box and k).  The frames come from the lifting-resolution
    depth maps and the intrinsics scaled to them with their inverse (scannet_2d3d.py:206-210, :38), per frame, on the device; `who`
    refuses images that disagree with the maps."""
    import numpy as np
    ldepth = depth if lift_depth is None else lift_depth
    F, H, W = ldepth.shape
    raw = _raw_frames(who, images, image_normalizer=image_normalizer is not None, channels_last=channels_last)
    if images.shape[0] != F or tuple(images.shape[1:3] if raw else images.shape[-2:]) != (H, W):
        raise RuntimeError(who + ': images (F,3,H,W) / (F,H,W,3) uint8 and the lifting depth (F,H,W) disagree: pass lift_depth at the images\' resolution')
    cam = (cam_matrix.detach().cpu().numpy() if torch.is_tensor(cam_matrix) else np.asarray(cam_matrix)).astype(np.float32)[..., :3, :3].copy()
    cam[..., 0, :] /= np.float32(depth.size(2) / W)  # `cam_matrix[0] /= resize_scale[0]` (:208-210)
    cam[..., 1, :] /= np.float32(depth.size(1) / H)
    kinv = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(cam))).to(dev).expand(F, 3, 3)  # float32, :38
    cam = torch.from_numpy(cam).to(dev).expand(F, 3, 3)
    return ldepth, lambda sel, points, pixel_box: {'depth': ldepth[sel].contiguous(), 'pose': pose[sel].contiguous(), 'points': points,
                                                   'cam_matrix': cam[sel].contiguous(), 'kinv': kinv[sel].contiguous(),
                                                   'pixel_box': pixel_box.contiguous(), 'k': int(k)}


def _raw_frames(who, images, **given):
    """True for raw (F,H,W,3) uint8 frames.  Float images are final: `who` refuses the image options `given` as true."""
    raw = images.dtype == torch.uint8
    if not raw and any(given.values()):
        raise RuntimeError('{}: {} need raw (F,H,W,3) uint8 frames; float images are final'.format(who, ' / '.join(n for n in given if given[n])))
    return raw


def _picked_views(images, depth, pose, sel, image_normalizer=None, channels_last=False, color_jitter=(), flip=0.0, generator=None):
    """The views `sel` (B,nv) of a frame store as a batch carries them: images, depth, pose [, flip].  Raw (F,H,W,3) uint8 images go
    through ops.prepare_frames with the loader's recipe -- the jitter and the flips are drawn here from `generator`, in this order --; float
    images are final (the caller has asked _raw_frames): a plain gather."""
    out = {'depth': depth[sel].contiguous(), 'pose': pose[sel].contiguous()}
    if images.dtype == torch.uint8:
        from . import augment as A
        factor, order = A.draw_color_jitter(tuple(sel.shape), color_jitter, sel.device, generator=generator) if color_jitter else (None, None)
        if flip:
            out['flip'] = A.draw_flip(tuple(sel.shape), flip, sel.device, generator=generator)
        out['images'] = ops.prepare_frames(images, sel.contiguous(), factor=factor, order=order, flip=out.get('flip'), normalizer=image_normalizer,
                                           channels_last=channels_last)
    else:
        out['images'] = images[sel].contiguous()
    return out


def bucket_size(n, min_nb_pts, max_bucket):
    """The padded size of a chunk of n points: the smallest rung >= max(n, min_nb_pts) of the ladder min_nb_pts x {1, 1.5, 2, 3, 4, 6, 8,
    12, 16, ...} (1.5 x rounded down; consecutive rungs differ by <= 1.5 x for min_nb_pts >= 2, so a chunk is padded to less than
    1.5 x max(n, min_nb_pts) rows), but never beyond max_bucket; a chunk above max_bucket keeps its size."""
    n, m = int(n), int(min_nb_pts)
    need = max(n, m)
    if n > max_bucket or m < 1:
        return need
    rung = m
    while rung < need:
        half = rung * 3 // 2
        rung = half if half >= need else rung * 2
    return max(need, min(rung, int(max_bucket)))


def plan_buckets(lengths, min_nb_pts=2048, batch_size=32, max_batch_points=32 * 8192, max_bucket=32768):
    """Batches for chunks of `lengths` points: every chunk is padded to bucket_size(n), the chunks are sorted by that size (ties keep
    their order) and cut into batches of at most min(batch_size, max(1, max_batch_points // size)) chunks of one size; a chunk above
    max_bucket is a batch of its own.  Host arithmetic only.  -> (batches: list of (size, [chunk numbers]), order: the chunk numbers in
    the batches' order)."""
    sizes = [bucket_size(n, min_nb_pts, max_bucket) for n in lengths]
    order = sorted(range(len(sizes)), key=lambda c: sizes[c])  # (stable)
    batches = []
    for c in order:
        N = sizes[c]
        cap = 1 if lengths[c] > max_bucket else min(int(batch_size), max(1, int(max_batch_points) // N))
        if batches and batches[-1][0] == N and len(batches[-1][1]) < cap and lengths[batches[-1][1][0]] <= max_bucket:
            batches[-1][1].append(c)
        else:
            batches.append((N, [c]))
    return batches, order


def prepare_scene_bucketed(points, depth, cam_matrix, pose, images, *, chunk_size, chunk_stride, chunk_thresh, chunk_margin, num_rgbd_frames, k,
                           min_nb_pts=2048, overlap=None, batch_size=32, lift_depth=None, num_base_pts=2000, radius=0.1, generator=None,
                           pad_seed=0, max_batch_points=32 * 8192, max_bucket=32768, image_normalizer=None, channels_last=False):
    """prepare_scene for a scene whose chunks have DIFFERENT sizes (the reference's test loop feeds every chunk with all its points):
    chunks of similar size share a batch after being padded to a common size (plan_buckets), with no per-chunk work on the host.
    Arguments as prepare_scene (raw uint8 frames with `image_normalizer` / `channels_last` included), `pad_seed` (an int) in place of
    `pad_generator`; single process.

    Padding is exact in eval mode: the duplicates are appended BEHIND a chunk's own points, so farthest point sampling picks the same
    indices (lowest index on ties), every ball holds the same distinct points, and the padded columns' logits are dropped by the vote.
    Steps: chunks.scene2chunks_csr (two kernels; the second and last device-to-host read of the preparation is the windows' counts),
    ops.pack_chunks (one launch writes every batch's points; the batches are views of one buffer), ONE ops.select_frames_batched call on
    bit rows (the overlap's and the chunker's base_bits: no membership matrix), then the frame gathers of prepare_scene.
    -> (chunk_batches, chunk_inds, n_pts, order): the batches sorted by size, chunk_inds -- views of the flat index list -- in THE
    BATCHES' ORDER, so `infer_scene(model, chunk_batches, chunk_inds, n_pts)` works as it stands; order[i] = the chunker's number
    (scene2chunks_legacy's position) of the i-th chunk.  The vote adds a point's logits in this order, not in the chunker's: sums differ
    from prepare_scene's in the last bits only."""
    csr = _scene_chunks(points, depth, cam_matrix, pose, overlap, num_rgbd_frames, chunk_size, chunk_stride, chunk_thresh, chunk_margin,
                        num_base_pts, radius, generator)
    lengths, n_pts, dev = csr['lengths'], points.size(0), points.device
    if not lengths:
        return [], [], n_pts, []
    batches, order, rows, picked, pixel_box, _ = _bucketed_rows(csr, points, 'prepare_scene_bucketed', min_nb_pts, batch_size, max_batch_points,
                                                                max_bucket, pad_seed)
    batch = _scene_batcher(dev, depth, cam_matrix, pose, images, lift_depth, 'prepare_scene_bucketed', k, image_normalizer, channels_last)
    chunk_batches, lo = [], 0
    for (N, members), pts in zip(batches, rows):
        hi = lo + len(members)
        chunk_batches.append(batch(picked[lo:hi], pts, pixel_box[lo:hi]))
        lo = hi
    chunk_inds = torch.split(csr['index'], lengths)
    return chunk_batches, [chunk_inds[c] for c in order], n_pts, order


def _bucketed_rows(csr, points, who, min_nb_pts, batch_size, max_batch_points, max_bucket, pad_seed):
    """What prepare_scene_bucketed, infer_scene_shared and infer_scene_2d share behind _scene_chunks: plan_buckets and ONE ops.pack_chunks
    launch.  -> (batches, order: plan_buckets' result; rows: every batch's padded points (B,3,N), views of one buffer; picked (C,nv) and
    pixel_box (C,4) in the batches' order; slot_base: _bucket_slots', the row of each chunk's first point, in the chunker's numbering)."""
    lengths = csr['lengths']
    batches, order, slot_base, out_len = _bucket_slots(lengths, who, min_nb_pts, batch_size, max_batch_points, max_bucket)
    packed = ops.pack_chunks(points.contiguous(), csr['index'], csr['offsets'], lengths, [3 * s for s in slot_base], out_len, seed=pad_seed)
    order_t = torch.tensor(order, dtype=torch.int64).to(points.device)
    return batches, order, _batch_views(packed, 3, batches, slot_base), csr['picked'][order_t], csr['pixel_box'][order_t], slot_base


def _bucket_slots(lengths, who, min_nb_pts, batch_size, max_batch_points, max_bucket):
    """The bucket and placement planning of every bucketed path (_bucketed_rows, infer_scene_3d): plan_buckets, and the batches laid one
    after the other in SLOTS (one slot = one padded point).  -> (batches, order: plan_buckets' result; slot_base, out_len: per chunk, in
    the chunker's numbering, its first slot and its padded size).  Host arithmetic only."""
    if min(lengths) < 1:
        raise RuntimeError(who + ': a chunk without points (chunk_thresh must be at least 1)')
    batches, order = plan_buckets(lengths, min_nb_pts=min_nb_pts, batch_size=batch_size, max_batch_points=max_batch_points, max_bucket=max_bucket)
    slot_base, out_len, at = [0] * len(lengths), [0] * len(lengths), 0
    for N, members in batches:
        for c in members:
            slot_base[c], out_len[c], at = at, N, at + N
    return batches, order, slot_base, out_len


def _batch_views(flat, channels, batches, slot_base):
    """Every batch's (B,channels,N) view of a flat buffer packed by _bucket_slots' placement."""
    return [flat[channels * slot_base[members[0]]:channels * (slot_base[members[0]] + len(members) * N)].view(len(members), channels, N)
            for N, members in batches]


def infer_scene_3d(model, points, colors=None, *, chunk_size=(1.5, 1.5), chunk_stride=0.5, chunk_thresh=1000, chunk_margin=(0.2, 0.2), min_nb_pts=2048,
                   use_color=None, batch_size=32, max_batch_points=32 * 8192, max_bucket=32768, pad_seed=0):
    """The sliding-window test of the 3D baselines (mvpnet/test_3d_chunks.py:106-167; configs/scannet/3d_baselines/pn2ssg_chunk.yaml,
    pn2ssg_rgb_chunk.yaml) from a scene's points [and colours]; the defaults are the script's.  Single process.
    model: a PN2SSG, or anything that maps {'points' (B,3,N) [, 'feature' (B,3,N)]} to {'seg_logit' (B,C,N)} and has `num_classes`; run in
    eval mode under no_grad, its mode is restored.  points (n,3) float32 on the device.  colors (n,3): uint8 as the stores hold them
    (the pack kernel writes colors / 255, scannet_3d.py:82) or float32 already divided by 255.  use_color: None = `model.in_channels == 3`
    (:95); a model that wants colours without `colors` raises before any launch.

    The reference feeds the chunks one at a time, every chunk with all its points, padded to min_nb_pts by transforms.Pad
    (transforms.py:136-148: uniform duplicates of the chunk's own points behind the originals).  Here chunks of similar size share a
    batch after padding to a common size by the same law (plan_buckets through _bucket_slots, as prepare_scene_bucketed; a duplicate
    carries its source point's colour) -- exact in eval mode, see prepare_scene_bucketed.  Steps: chunks.scene2chunks_csr without base
    points (its two host reads -- the scene's extent and the windows' counts -- are the only ones), ONE ops.pack_cloud launch writes every
    batch's points and features, _forward_batches, _vote_chunk_logits (the atomics-free vote, adding in the batches' order).
    -> mean logits (n,C), labels (n,) with C where no chunk holds the point, counts (n,) int32.  A scene with no kept window gives zeros,
    labels all C and counts zero, and nothing goes through the model."""
    _check_scene_points('infer_scene_3d', points)
    net = _unwrap(model)
    dev, n_pts, num_classes = points.device, points.size(0), int(net.num_classes)
    use_color = (getattr(net, 'in_channels', 0) == 3) if use_color is None else bool(use_color)
    source = {}
    if use_color:
        if colors is None:
            raise RuntimeError('infer_scene_3d: the model reads colours (in_channels = 3 / use_color) but no colors were given')
        if colors.dim() != 2 or tuple(colors.shape) != (n_pts, 3) or colors.dtype not in (torch.uint8, torch.float32) or colors.device != dev:
            raise RuntimeError('infer_scene_3d: colors must be (n,3) uint8, or float32 already divided by 255, on the points\' device')
        source = {'colors' if colors.dtype == torch.uint8 else 'feature': colors.contiguous()}
    csr = CH.scene2chunks_csr(points, chunk_size, chunk_stride, thresh=chunk_thresh, margin=chunk_margin)
    lengths = csr['lengths']
    if not lengths:
        return _no_prediction(n_pts, num_classes, dev)
    batches, order, slot_base, out_len = _bucket_slots(lengths, 'infer_scene_3d', min_nb_pts, batch_size, max_batch_points, max_bucket)
    flat_points, flat_feature = ops.pack_cloud(points.contiguous(), csr['index'], csr['offsets'], lengths, slot_base, out_len, seed=pad_seed, **source)
    chunk_batches = [{'points': p} for p in _batch_views(flat_points, 3, batches, slot_base)]
    if use_color:
        for b, f in zip(chunk_batches, _batch_views(flat_feature, 3, batches, slot_base)):
            b['feature'] = f
    with eval_mode(model):
        outs = _forward_batches(model, chunk_batches)
    chunk_inds = torch.split(csr['index'], lengths)
    return _vote_chunk_logits(outs, [chunk_inds[c] for c in order], n_pts, len(order), num_classes)


def ensemble_scene(logits_per_model, want_prob=True):
    """The model ensemble of mvpnet/ensemble.py:45-49 on a scene: logits_per_model: the `mean` logits (n,C) that 1..8 models' runs of any
    whole-scene test path (infer_scene, infer_scene_shared, infer_scene_2d, infer_scene_votes, infer_scene_3d) returned for ONE scene.
    -> (prob (n,C): the sum of the models' softmaxes, or None; label (n,) int64: its argmax, first maximum).  One launch
    (ops.ensemble_softmax), no stacked copy.  Unlike a test path's labels these have no "no prediction" class: a point no chunk holds has
    zero logits in every model, hence equal probabilities and label 0, exactly as the reference's script treats its saved logits.  Raw
    ids for a submission: `scannet_to_nyu40[label]`, plain tensor indexing."""
    return ops.ensemble_softmax(logits_per_model, want_prob=want_prob)


def plan_store_groups(frames_of_batch, max_frames):
    """Runs of consecutive batches that share one feature store (infer_scene_shared).  frames_of_batch: per batch, the frames its chunks
    picked (any iterable of ints, repeats allowed); max_frames: the most distinct frames a store may hold.  Greedy: a run grows while the
    union of its batches' frames stays within max_frames; a single batch that needs more is a run of its own.  Host arithmetic only; the
    batches themselves never depend on the cap.  -> list of (first batch, one past the last, the run's distinct frames ascending)."""
    max_frames = int(max_frames)
    if max_frames < 1:
        raise RuntimeError('plan_store_groups: max_frames must be at least 1 (a store that cannot hold one frame)')
    runs, lo, hi, union = [], 0, 0, set()
    for frames in frames_of_batch:
        frames = {int(f) for f in frames}
        if hi > lo and len(union | frames) > max_frames:
            runs.append((lo, hi, sorted(union)))
            lo, union = hi, set()
        union |= frames
        hi += 1
    if hi > lo:
        runs.append((lo, hi, sorted(union)))
    return runs


def _frames_through(net_2d, key, images, image_normalizer, channels_last):
    """-> run(frames): the frames (b,) int64 on the device, as the 2D network reads them (_test_frames), through net_2d -> its `key` output."""
    return lambda frames: net_2d({'image': _test_frames(images, frames, image_normalizer, channels_last)})[key]


def _frame_store(distinct, F, H, W, frame_batch, run, who, dev, channels=None, dtype=None):
    """Every distinct picked frame through the 2D network once (infer_scene_shared per run, infer_scene_2d per scene).  distinct: the
    frames, an ascending host list of ints in [0, F); run(frames (b,) int64 on `dev`) -> (b,C,H,W) float32, called with at most frame_batch
    frames at a time; channels: C, or None = the first output's.  `who` refuses any other output.
    dtype: None = a float32 store of a float32 network; torch.bfloat16 / torch.float16 = a store of that type, of a network that returns
    float32 -- the copy into the store rounds each value once, to nearest even -- or exactly that type (copied as it is).
    -> (store (U,H,W,C) float32 or `dtype` -- channels-last memory whatever the network writes: the copy into the store makes a pixel's C values one
    contiguous row, and store.permute(0, 3, 1, 2) is the (U,C,H,W) tensor --, slot_of (F,) int32: a frame's place in the store, -1 for a
    frame that is not in it)."""
    if dtype not in (None, torch.bfloat16, torch.float16):
        raise RuntimeError('{}: the store is float32 (None), torch.bfloat16 or torch.float16'.format(who))
    accepted = (torch.float32,) if dtype is None else (torch.float32, dtype)
    frames = torch.tensor(distinct, dtype=torch.int64).to(dev)
    store = None
    for lo in range(0, len(distinct), int(frame_batch)):
        part = frames[lo:lo + int(frame_batch)]
        out = run(part)
        if not torch.is_tensor(out) or out.dim() != 4 or out.dtype not in accepted \
                or tuple(out.shape) != (part.numel(), out.size(1) if channels is None else channels, H, W):
            raise RuntimeError('{}: net_2d must return a float32{} (b,{},{},{}) tensor for b frames: the lifting maps\' size'.format(
                who, '' if dtype is None else ' or {}'.format(dtype), 'C' if channels is None else channels, H, W))
        if store is None:
            channels = out.size(1)
            store = torch.empty((len(distinct), H, W, channels), dtype=torch.float32 if dtype is None else dtype, device=dev)
        store[lo:lo + part.numel()].permute(0, 3, 1, 2).copy_(out)
    slot_of = torch.full((F,), -1, dtype=torch.int32, device=dev)
    slot_of[frames] = torch.arange(len(distinct), dtype=torch.int32, device=dev)
    return store, slot_of


def infer_scene_shared(model, points, depth, cam_matrix, pose, images, *, chunk_size, chunk_stride, chunk_thresh, chunk_margin, num_rgbd_frames, k,
                       min_nb_pts=2048, overlap=None, lift_depth=None, num_base_pts=2000, radius=0.1, generator=None, pad_seed=0, batch_size=32,
                       max_batch_points=32 * 8192, max_bucket=32768, image_normalizer=None, channels_last=False, frame_batch=32,
                       max_store_bytes=8 << 30, store_dtype=None):
    """The whole-scene test of MVPNet (mvpnet/test_mvpnet_3d.py:142-174) from a scene's raw arrays with every frame through the 2D network
    ONCE: `infer_scene(model, *prepare_scene_bucketed(...)[:3])` -- same chunks, same frames, same batches in the same order, same padded
    points, same kernels behind the lift -- without its (B,nv,3,H,W) images per batch.  Single process.
    model: an MVPNet3D; run in eval mode under no_grad, its mode is restored.  The other arguments are prepare_scene_bucketed's;
    frame_batch: frames per forward of the 2D network; max_store_bytes: the most memory a feature store may take.
    store_dtype: None = a float32 store; torch.bfloat16 / torch.float16 = a store of that type, which holds twice the frames in the same
    bytes and is lifted from as it is (ops.lift_store widens the rows it gathers, exactly).  With a float32 2D network this is a LOSSY
    opt-in: every feature is rounded once, to nearest even, on its way into the store.  A network that already produces that type
    (UNetResNet34.frozen_inference(compute_dtype, feature_dtype)) loses nothing.

    Neighbouring chunks pick largely the same frames, and in eval mode a frame's feature map does not depend on its batch neighbours (with
    MIOpen its last bits may depend on the batch SIZE; an elementwise network's do not).  The batches are cut into runs of consecutive
    batches whose distinct frames fit one store (plan_store_groups, max_store_bytes // (H*W*C*itemsize) frames; host arithmetic on the picked
    table -- the one device-to-host read beyond _scene_chunks' own --; the batch plan never depends on the cap).  Per run the distinct
    frames go through model.net_2d once each (raw uint8 frames through ops.prepare_frames first, as in infer_scene_2d) into one
    channels-last store (U,H,W,C); the run's batches carry `feature_store` / `view_slot` in place of `images`, so MVPNet3D lifts
    with ops.lift_store -- no 2D forward, no channels-last copy per batch --, the next batch's geometry prefetched as infer_scene does; the
    store is released before the next run's is made.  A frame two runs share runs once per run.
    -> mean logits (n_pts,C), labels (n_pts,) with C where no chunk holds the point, counts (n_pts,) int32, as infer_scene.  A scene with
    no kept window gives zeros, labels all C, counts zero, and nothing goes through the 2D network."""
    dev, n_pts = points.device, points.size(0)
    if frame_batch < 1:
        raise RuntimeError('infer_scene_shared: frame_batch must be at least 1')
    if store_dtype not in (None, torch.bfloat16, torch.float16):
        raise RuntimeError('infer_scene_shared: store_dtype must be None (float32), torch.bfloat16 or torch.float16')
    net = _unwrap(model)
    num_classes, C = int(net.net_3d.num_classes), int(net.feat_aggreg.in_channels)
    csr = _scene_chunks(points, depth, cam_matrix, pose, overlap, num_rgbd_frames, chunk_size, chunk_stride, chunk_thresh, chunk_margin,
                        num_base_pts, radius, generator)
    lengths = csr['lengths']
    if not lengths:
        return _no_prediction(n_pts, num_classes, dev)
    ldepth, geometry = _scene_geometry(dev, depth, cam_matrix, pose, images, lift_depth, 'infer_scene_shared', k, image_normalizer, channels_last)
    F, H, W = ldepth.shape
    batches, order, rows, picked, pixel_box, _ = _bucketed_rows(csr, points, 'infer_scene_shared', min_nb_pts, batch_size, max_batch_points, max_bucket,
                                                                pad_seed)
    picked_host = picked.cpu().tolist()  # (the one read)
    chunk_batches, sels, frames_of_batch, lo = [], [], [], 0
    for (_, members), pts in zip(batches, rows):  # prepare_scene_bucketed's batches without `images`
        hi = lo + len(members)
        chunk_batches.append(geometry(picked[lo:hi], pts, pixel_box[lo:hi]))
        sels.append(picked[lo:hi])
        frames_of_batch.append({f for row in picked_host[lo:hi] for f in row})
        lo = hi
    runs = plan_store_groups(frames_of_batch, int(max_store_bytes) // (H * W * C * (4 if store_dtype is None else 2)))
    run_of_batch = {first: r for r, (first, _, _) in enumerate(runs)}
    run_2d = _frames_through(net.net_2d, 'feature', images, image_normalizer, channels_last)
    state = {'store': None, 'slot_of': None}

    def ready(i, batch):
        """Batch i as the model takes it; the first batch of a run makes the run's store (the previous one is released first)."""
        if i in run_of_batch:
            state['store'] = state['slot_of'] = None
            state['store'], state['slot_of'] = _frame_store(runs[run_of_batch[i]][2], F, H, W, frame_batch, run_2d, 'infer_scene_shared', dev, C,
                                                            store_dtype)
        return dict(batch, feature_store=state['store'], view_slot=state['slot_of'][sels[i]].contiguous())

    try:
        with eval_mode(model):
            outs = _forward_batches(model, chunk_batches, ready)
    finally:
        state.clear()
    chunk_inds = torch.split(csr['index'], lengths)
    return _vote_chunk_logits(outs, [chunk_inds[c] for c in order], n_pts, len(order), num_classes)


def scene_from_rgbd(depth, cam_matrix, pose, images=None, *, voxel=0.05, min_samples=1, max_voxels=None, depth_min=None, depth_max=None):
    """The `points` every whole-scene call takes, made from the recording itself (new: the reference reads the vertices of ScanNet's offline
    mesh, mvpnet/data/preprocess/preprocess.py:204): the voxel-grid fusion of the un-projected depth pixels, ops.fuse_cloud.
    depth (F,h,w) float32 metres or (u)int16 millimetres on the device; cam_matrix (3,3) / (4,4) intrinsics OF THE DEPTH MAPS' RESOLUTION,
    array or tensor, (F,3,3) for per-frame intrinsics, inverted as chunks.compute_rgbd_overlap does; pose (F,4,4) float32; images
    (F,h,w,3) uint8 colour frames of the depth maps' size, or None; voxel: metres; min_samples: pixels a voxel needs to become a point;
    max_voxels: None = the pixel count; depth_min / depth_max: metres, pixels outside are ignored.
    -> {'points' (n,3) float32, 'colors' (n,3) uint8 or None, 'count' (n,) int32, 'pixel_point' (F,h,w) int32: each pixel's point, -1 where
    it has none}.  Exact and independent of the frames' order.  A fused cloud is denser where frames overlap and sparser far from the
    camera than a mesh's vertices; what that does to weights trained on mesh vertices has not been measured."""
    import numpy as np
    if not torch.is_tensor(depth):
        raise RuntimeError('scene_from_rgbd: depth must be a (F,h,w) tensor')
    kinv = torch.from_numpy(np.ascontiguousarray(CH._kinv_of(cam_matrix))).to(depth.device)
    pose = pose.contiguous() if torch.is_tensor(pose) else pose
    points, colors, count, pixel_point = ops.fuse_cloud(depth.contiguous(), kinv, pose, None if images is None else images.contiguous(), voxel=voxel,
                                                        max_voxels=max_voxels, min_samples=min_samples, depth_min=depth_min, depth_max=depth_max)
    return {'points': points, 'colors': colors, 'count': count, 'pixel_point': pixel_point}


def infer_rgbd(model, depth, cam_matrix, pose, images, *, voxel, min_samples=1, max_voxels=None, depth_min=None, depth_max=None, **scene_kwargs):
    """An RGB-D recording labelled from its own frames: scene_from_rgbd, then infer_scene_shared on the fused points with the same frames.
    model, depth, cam_matrix, pose, images and scene_kwargs are infer_scene_shared's (chunk_size, chunk_stride, ..., lift_depth,
    image_normalizer, ...); voxel, min_samples, max_voxels, depth_min, depth_max are scene_from_rgbd's.  The cloud takes its colours from
    `images` when they are raw (F,h,w,3) uint8 frames of the depth maps' size, and has none otherwise.
    -> scene_from_rgbd's dict + 'mean' (n,C), 'label' (n,) int64, 'vote_count' (n,) int32 -- infer_scene_shared's three -- and
    'label_frames' (F,h,w) int64: the points' labels read back through pixel_point, C ("no prediction") where pixel_point is -1."""
    raw = torch.is_tensor(images) and images.dtype == torch.uint8 and images.dim() == 4 and tuple(images.shape[:3]) == tuple(depth.shape)
    cloud = scene_from_rgbd(depth, cam_matrix, pose, images if raw else None, voxel=voxel, min_samples=min_samples, max_voxels=max_voxels,
                            depth_min=depth_min, depth_max=depth_max)
    mean, label, votes = infer_scene_shared(model, cloud['points'], depth, cam_matrix, pose, images, **scene_kwargs)
    num_classes = mean.size(1)
    pp = cloud['pixel_point'].long()
    label_frames = torch.where(pp >= 0, label[pp.clamp(min=0)] if label.numel() else pp, torch.full((), num_classes, dtype=torch.int64, device=pp.device))
    return dict(cloud, mean=mean, label=label, vote_count=votes, label_frames=label_frames)


def infer_scene_2d(model, points, depth, cam_matrix, pose, images, *, chunk_size, chunk_stride, chunk_thresh, chunk_margin, num_rgbd_frames, k,
                   overlap=None, lift_depth=None, num_base_pts=2000, radius=0.1, generator=None, image_normalizer=None, channels_last=False,
                   frame_batch=32):
    """The whole-scene test of the 2D baseline (mvpnet/test_2d_chunks.py:119-157) from a scene's raw arrays: the 2D network's per-pixel
    class logits lifted to every chunk's points through the pixel k-NN, averaged over k and voted into the scene.  Single process.
    model: an MVPNet2D, or anything with a `.net_2d` that maps {'image' (F,3,H,W)} to {'seg_logit' (F,C,H,W)}; run in eval mode under
    no_grad, its mode is restored.  The other arguments are prepare_scene's (raw (F,H,W,3) uint8 frames with `image_normalizer` /
    `channels_last` included); frame_batch: frames per forward of the 2D network.

    The reference feeds the chunks one by one, each with its own num_rgbd_frames frames, so the 2D network sees a frame once per chunk
    that picked it.  In eval mode a frame's logits do not depend on its batch neighbours: here the network runs ONCE per distinct picked
    frame and writes into one channels-last logit store (_frame_store, infer_scene_shared's); the pixel k-NN runs per chunk against that
    chunk's own views and box, in size-bucketed batches (_bucketed_rows with min_nb_pts = 1: there is no FPS to pad for; the padded rows
    are searched and never read), into one flat index buffer; ops.lift_vote then goes from every scene point through its chunk positions
    and their k pixel ids to the logit rows in one launch, adding in the chunker's chunk order -- the reference's -- and ops.vote_finish
    divides and labels.  One device-to-host read beyond _scene_chunks': the picked table, from which the host lists the distinct frames.
    -> mean logits (n_pts,C), labels (n_pts,) with C where no chunk holds the point, counts (n_pts,) int32.  A scene with no kept window
    gives zeros, labels all C and counts zero (C: net_2d.num_classes, else one frame is run to learn it)."""
    n_pts = points.size(0)
    parts = _scene_2d_inputs(model, points, depth, cam_matrix, pose, images, chunk_size=chunk_size, chunk_stride=chunk_stride, chunk_thresh=chunk_thresh,
                             chunk_margin=chunk_margin, num_rgbd_frames=num_rgbd_frames, k=k, overlap=overlap, lift_depth=lift_depth,
                             num_base_pts=num_base_pts, radius=radius, generator=generator, image_normalizer=image_normalizer,
                             channels_last=channels_last, frame_batch=frame_batch)
    if 'logit' not in parts:
        return _no_prediction(n_pts, parts['num_classes'], points.device)
    total, count = ops.lift_vote(parts['logit'], parts['view_frame'], parts['knn'], parts['knn_base'], parts['chunk_inds'], n_pts)
    return (*ops.vote_finish(total, count), count)


def _scene_2d_inputs(model, points, depth, cam_matrix, pose, images, *, chunk_size, chunk_stride, chunk_thresh, chunk_margin, num_rgbd_frames, k,
                     overlap, lift_depth, num_base_pts, radius, generator, image_normalizer, channels_last, frame_batch):
    """infer_scene_2d up to the vote: -> {'num_classes'} for a scene without a kept window, else what ops.lift_vote takes -- logit (U,C,H,W)
    in channels-last memory: _frame_store's store of the distinct picked frames' logits; view_frame (num_chunks,nv) int32: its slot_of at
    the picked table; knn (R,k) int64 and knn_base: the chunks' rows, batch after batch (_bucketed_rows' placement); chunk_inds in the
    chunker's order -- and picked (num_chunks,nv).  The picked table is read to the host once, for the distinct frames."""
    from . import _lib as L
    dev, nv, k = points.device, int(num_rgbd_frames), int(k)
    _check_scene_points('infer_scene_2d', points)
    if not 1 <= k <= ops.vote.MAX_K or frame_batch < 1:
        raise RuntimeError('infer_scene_2d: needs 1 <= k <= {} and frame_batch >= 1'.format(ops.vote.MAX_K))
    ldepth, geometry = _scene_geometry(dev, depth, cam_matrix, pose, images, lift_depth, 'infer_scene_2d', k, image_normalizer, channels_last)
    F, H, W = ldepth.shape
    net_2d = _unwrap(model).net_2d
    run_2d = _frames_through(net_2d, 'seg_logit', images, image_normalizer, channels_last)
    csr = _scene_chunks(points, depth, cam_matrix, pose, overlap, num_rgbd_frames, chunk_size, chunk_stride, chunk_thresh, chunk_margin,
                        num_base_pts, radius, generator)
    lengths = csr['lengths']
    with eval_mode(model):
        if not lengths:
            C = getattr(net_2d, 'num_classes', None)
            return {'num_classes': int(run_2d(torch.zeros(1, dtype=torch.int64, device=dev)).size(1)) if C is None else int(C)}
        # pixel k-NN per chunk, in size-bucketed batches (no FPS to pad for: min_nb_pts = 1), into one flat buffer
        batches, _, rows, picked, pixel_box, knn_base = _bucketed_rows(csr, points, 'infer_scene_2d', 1, 32, 32 * 8192, 32768, 0)
        distinct = sorted({f for row in csr['picked'].cpu().tolist() for f in row})  # (the one read)
        store, slot_of = _frame_store(distinct, F, H, W, frame_batch, run_2d, 'infer_scene_2d', dev)
        knn = torch.empty((sum(N * len(members) for N, members in batches), k), dtype=torch.int64, device=dev)
        lo = 0
        for (N, members), pts in zip(batches, rows):
            B, pts = len(members), pts.transpose(1, 2).contiguous()  # (B,N,3)
            d = geometry(picked[lo:lo + B], pts, pixel_box[lo:lo + B])
            xyz, mask = ops.unproject(d['depth'], d['kinv'], d['pose'], d['pixel_box'])
            mask = mask.to(torch.uint8)
            L.call('mvp_pixel_knn_projective_f32', pts, L.ptr(xyz), L.ptr(mask), L.ptr(pts), L.ptr(d['cam_matrix']), L.ptr(d['pose']), B, nv, H, W, N, k,
                   L.ptr_at(knn, knn_base[members[0]] * k), None)
            lo += B
        return {'logit': store.permute(0, 3, 1, 2), 'view_frame': slot_of[csr['picked']], 'knn': knn, 'knn_base': knn_base,
                'chunk_inds': list(torch.split(csr['index'], lengths)), 'picked': csr['picked'], 'num_classes': int(store.size(3))}


def sample_train_batch(store, scene_of_chunk, *, nb_pts, num_rgbd_frames, k, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2), chunk_thresh=0.3,
                       num_tries=10, generator=None, color_jitter=(), image_normalizer=None, flip=0.0, channels_last=False):
    """One TRAINING batch from scenes resident on the device: what a batch of `ScanNet2D3DChunks.__getitem__` calls collates to
    (mvpnet/data/scannet_2d3d.py:323-398 with get_rgbd_data's frame choice, :199-221), without a host synchronisation.
    store: dict of device tensors --
        points (Ntot,3) float32, seg_label (Ntot,) int64 (mapped, negative = unlabelled), scene_offsets (S+1,) int64: the scenes, one
        after the other; base_point_ind (S,nbp) int64 inside each scene; overlap_bits (Ftot,W) int32 bit rows (ops.rgbd_overlap(...,
        packed=True) per scene, concatenated) and frame_offsets (S+1,) int64; depth (Ftot,H,W), images (Ftot,3,H,W) [or raw, below], pose (Ftot,4,4) at
        the lifting resolution; cam / kinv (S,3,3) float32: every scene's intrinsics of that resolution and their inverse.
    scene_of_chunk (B,) int64 on the device: the dataset indices of the batch.
    chunks.sample_train_chunks draws the chunks (one call), ops.select_frames_batched with the scenes' frame ranges picks the frames
    (one launch), the rest are gathers.  -> the dict MVPNet3D._forward and SegLoss read: images (B,nv,3,H,W), points (B,3,nb_pts),
    seg_label (B,nb_pts), depth (B,nv,H,W), cam_matrix / kinv (B,nv,3,3), pose (B,nv,4,4), pixel_box (B,4) = chunk_box -/+ fl32(0.1) in
    float32 (:274-281), k.  augment.DeviceAugmentation applies to it as to any batch.

    A RAW store -- images (Ftot,H,W,3) uint8, as the PNGs decode: a quarter of the float store's bytes -- gets the loader's image recipe
    on the device as well (:241-252, :293-296; ops.prepare_frames on the picked frames): color_jitter = the YAML's (brightness, contrast,
    saturation), drawn per frame by augment.draw_color_jitter; image_normalizer = the YAML's (mean, std); flip = the probability of
    mirroring a view, drawn by augment.draw_flip -- the batch then carries 'flip' (B,nv) uint8, which MVPNet3D / ops.lift consume, so
    DeviceAugmentation is left with z_rot only; channels_last: images with (B,nv,H,W,3) memory.  All draws come from `generator`, behind
    the chunks' draws, in this order: jitter, flip.  A float store is final: it takes none of the four."""
    ch = CH.sample_train_chunks(store['points'], store['seg_label'], store['scene_offsets'], scene_of_chunk, nb_pts, chunk_size=chunk_size,
                                chunk_margin=chunk_margin, chunk_thresh=chunk_thresh, num_tries=num_tries,
                                base_point_ind=store['base_point_ind'], generator=generator)
    return assemble_train_batch(store, scene_of_chunk, ch, num_rgbd_frames, k, color_jitter=color_jitter, image_normalizer=image_normalizer, flip=flip,
                                channels_last=channels_last, generator=generator)


def assemble_train_batch(store, scene_of_chunk, ch, num_rgbd_frames, k, *, color_jitter=(), image_normalizer=None, flip=0.0, channels_last=False,
                         generator=None):
    """sample_train_batch behind the draw: `ch` is ops.sample_chunks' result for the store's scenes (with base_bits); the keyword
    arguments are sample_train_batch's, for a raw uint8 store."""
    _raw_frames('assemble_train_batch', store['images'], color_jitter=color_jitter, image_normalizer=image_normalizer is not None, flip=flip,
                channels_last=channels_last)
    nv = int(num_rgbd_frames)
    fo = store['frame_offsets']
    begin = fo[scene_of_chunk]
    count = fo[scene_of_chunk + 1] - begin
    picked = ops.select_frames_batched(store['overlap_bits'], ch['base_bits'], nv, frame_begin=begin, frame_count=count)  # (B,nv) global rows
    B, box = scene_of_chunk.numel(), ch['chunk_box']
    return {**_picked_views(store['images'], store['depth'], store['pose'], picked, image_normalizer, channels_last,
                            color_jitter, flip, generator), 'points': ch['points'], 'seg_label': ch['seg_label'],
            'cam_matrix': store['cam'][scene_of_chunk][:, None].expand(B, nv, 3, 3).contiguous(),
            'kinv': store['kinv'][scene_of_chunk][:, None].expand(B, nv, 3, 3).contiguous(),
            'pixel_box': torch.cat([box[:, :2] - 0.1, box[:, 2:] + 0.1], dim=1), 'k': int(k)}


def sample_train_batch_2d(store, picked, *, resize=None, color_jitter=(), image_normalizer=None, flip=0.0, label_mapping=None, channels_last=False,
                          generator=None):
    """One batch of the 2D stage (configs/scannet/unet_resnet34.yaml, train_2d.py) from frames resident on the device: what a batch of
    `ScanNet2D.__getitem__` calls collates to (mvpnet/data/scannet_2d.py:146-181), without a host synchronisation.
    store: dict of device tensors -- images (Ftot,H,W,3) uint8 RGB and labels (Ftot,H,W) uint16 raw ids, as the PNGs decode.
    picked (B,) int64 on the device: the frames of the batch (a sampler's, or augment.draw_frames').
    The reference's order: resize -> jitter -> flip -> `/ 255.` -> normalise.  resize: the YAML's (w, h) or None; when it differs from the
    store's size, ops.resize_frames (Pillow's BILINEAR, bit for bit) makes the uint8 frames of that size and the labels are read through
    Pillow's NEAREST indices; ops.prepare_frames then runs on those frames with color_jitter = the YAML's (brightness, contrast,
    saturation) (augment.draw_color_jitter), flip = the probability of mirroring a frame (augment.draw_flip) and image_normalizer = the
    YAML's (mean, std); ops.prepare_labels gets the SAME flip draw and label_mapping ((T,) int64 on the device:
    config.scannet_label_mapping; None keeps the raw ids).  channels_last: images with (B,h,w,3) memory.  All draws come from
    `generator`, in this order: jitter, flip.
    -> {'image': (B,3,h,w) float32, 'seg_label': (B,h,w) int64}: what UNetResNet34 and SegLoss read."""
    from . import augment as A
    images, labels = store['images'], store['labels']
    if images.dim() != 4 or labels.dim() != 3 or tuple(labels.shape) != tuple(images.shape[:3]):
        raise RuntimeError('sample_train_batch_2d: images (Ftot,H,W,3) uint8 and labels (Ftot,H,W) uint16 must describe the same frames')
    if picked.dim() != 1:
        raise RuntimeError('sample_train_batch_2d: picked must be (B,)')
    size = _resize_target(resize, images.size(2), images.size(1))
    dev, B = images.device, picked.numel()
    factor, order = A.draw_color_jitter(B, color_jitter, dev, generator=generator) if color_jitter else (None, None)
    flips = A.draw_flip(B, flip, dev, generator=generator) if flip else None
    image = _sized_frames(images, picked, size, factor=factor, order=order, flip=flips, normalizer=image_normalizer, channels_last=channels_last)
    return {'image': image, 'seg_label': ops.prepare_labels(labels, picked, size=size, flip=flips, mapping=label_mapping)}


def _resize_target(resize, W, H):
    """The YAML's resize (w, h) -> the size to resize (W,H) frames to, or None when there is nothing to do: no resize, or the frames' own."""
    if resize is None or len(resize) == 0 or (int(resize[0]), int(resize[1])) == (W, H):
        return None
    return int(resize[0]), int(resize[1])


def _sized_frames(images, picked, size, *, factor=None, order=None, flip=None, normalizer, channels_last):
    """The frames `picked` (B,) of a raw (Ftot,H,W,3) uint8 store as the 2D network reads them: ops.resize_frames to `size` (_resize_target's)
    when it is not None, then ops.prepare_frames with the given jitter, flip and normaliser."""
    if size is not None:
        images, picked = ops.resize_frames(images, picked, size), _arange(picked.numel(), images.device)
    return ops.prepare_frames(images, picked, factor=factor, order=order, flip=flip, normalizer=normalizer, channels_last=channels_last)


_ARANGE = {}  # (device, n) -> arange(n) int64 on the device: made once, so a later batch launches nothing for it


def _arange(n, dev):
    t = _ARANGE.get((dev, n))
    if t is None:
        t = _ARANGE[(dev, n)] = torch.arange(n, dtype=torch.int64, device=dev)
    return t


def sample_train_batch_3d(store, scene_of_row, *, dataset, nb_pts, use_color=False, z_rot=None, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2),
                          chunk_thresh=0.3, num_tries=10, generator=None):
    """One batch of a 3D baseline (configs/scannet/3d_baselines/*.yaml) from scenes resident on the device: what a batch of
    `ScanNet3DChunks.__getitem__` / `ScanNet3DScene.__getitem__` calls with the transform `CropPad(nb_pts)` [+ `RandomRotateZ`] collates to
    (mvpnet/data/scannet_3d.py:135-221, mvpnet/data/transforms.py:64-133), without a host synchronisation.
    store: dict of device tensors -- points (Ntot,3) float32, seg_label (Ntot,) int64 (mapped, negative = unlabelled), scene_offsets (S+1,)
        int64: the scenes, one after the other; colors (Ntot,3) uint8 for use_color.
    scene_of_row (B,) int64 on the device: the dataset indices of the batch.
    dataset: 'ScanNet3DChunks' -- chunks.sample_train_chunks(..., bounds_f64=True) draws a chunk per row (chunk_size, chunk_margin,
        chunk_thresh, num_tries: the YAML's DATASET.ScanNet3DChunks; nb_pts <= 8192) -- or 'ScanNet3DScene' -- chunks.sample_train_scenes
        crops or pads the whole scene (nb_pts <= 65536; the chunk arguments are not used).  ops.gather_cloud then reads the store once.
    z_rot: None -- the validation recipe, points are copied -- or (low, high) in radians, RandomRotateZ's (-pi, pi): one matrix per row
        (augment.draw_z_rotation), applied as `points @ R.T` in float32.
    All draws come from `generator`, in this order: the sampler's (ScanNet3DChunks: the centres, then the seed; ScanNet3DScene: the
    seed), then the angles.
    -> what PN2SSG and SegLoss read: points (B,3,nb_pts) float32, seg_label (B,nb_pts) int64 [, feature (B,3,nb_pts) float32 = colors / 255]
    + the draws: choice (B,nb_pts) int64 inside each row's scene [, z_rot (B,3,3) float32]."""
    from . import augment as A
    points, offsets = store['points'], store['scene_offsets']
    if dataset == 'ScanNet3DChunks':
        choice = CH.sample_train_chunks(points, store['seg_label'], offsets, scene_of_row, nb_pts, chunk_size=chunk_size, chunk_margin=chunk_margin,
                                        chunk_thresh=chunk_thresh, num_tries=num_tries, bounds_f64=True, generator=generator)['choice']
    elif dataset == 'ScanNet3DScene':
        choice = CH.sample_train_scenes(offsets, scene_of_row, nb_pts, Ntot=points.size(0), generator=generator)['choice']
    else:
        raise ValueError("sample_train_batch_3d: dataset must be 'ScanNet3DChunks' or 'ScanNet3DScene', not {!r}".format(dataset))
    rot = None
    if z_rot is not None:
        low, high = z_rot
        rot = A.draw_z_rotation(scene_of_row.numel(), low, high, device=points.device, generator=generator)
    out = ops.gather_cloud(points, offsets, scene_of_row, choice, seg_label=store['seg_label'], colors=store['colors'] if use_color else None, rot=rot)
    out['choice'] = choice
    if rot is not None:
        out['z_rot'] = rot
    return out


def val_batches(num_scenes, *, batch_size, repeats, sample, device):
    """The validation loader of stage two and of the 3D baselines (mvpnet/data/build.py:28-47) as a generator: the order of
    RepeatSampler (common/utils/sampler.py:36-45: range(num_scenes), `repeats` times over, VAL.REPEATS) cut into batches of `batch_size`
    with the last one partial (drop_last=False), each handed to `sample` as a (b,) int64 tensor on `device` -- the dataset indices of
    the batch, what scene.sample_train_batch / sample_train_batch_3d take as scene_of_chunk / scene_of_row.  `sample` is the caller's
    closure over one of the two with the validation recipe (no flip, jitter or rotation; the baselines' VAL.AUGMENTATION CropPad is
    sample_train_batch_3d's nb_pts); what it returns is yielded.  The whole order is ONE host-to-device copy, made before the first batch; mvpnet3d.validate consumes the
    generator one batch ahead."""
    num_scenes, batch_size, repeats = int(num_scenes), int(batch_size), int(repeats)
    if num_scenes < 0 or batch_size < 1 or repeats < 0:
        raise ValueError('val_batches: num_scenes >= 0, batch_size >= 1, repeats >= 0 expected')
    order = torch.arange(num_scenes, dtype=torch.int64).repeat(repeats).to(device)
    for lo in range(0, order.numel(), batch_size):
        yield sample(order[lo:lo + batch_size])


def label_weights_2d(store, frames=None, *, resize=None, label_mapping, num_classes=20):
    """The 2D class weights of mvpnet/data/preprocess/compute_label_weights.py:34-49 (`compute_2d_weights`) from label frames resident on
    the device: one ops.label_histogram launch over `frames` -- (n,) int64 on the device, None for all; the reference takes every 100th
    frame, `torch.arange(0, Ftot, 100)` -- at the YAML's resize (w, h) through label_mapping, then metric.label_log_weights on the counts
    (the read of num_classes integers is the only synchronisation).  -> (num_classes,) float32 NumPy array, what the script saves."""
    labels = store['labels']
    size = _resize_target(resize, labels.size(2), labels.size(1))
    return metric.label_log_weights(ops.label_histogram(labels, num_classes, picked=frames, size=size, mapping=label_mapping))


def label_weights_3d(seg_label, *, num_labels=41, class_ids=tuple(metric.EVAL_CLASS_IDS)):
    """The 3D class weights of compute_label_weights.py:16-31 (`compute_3d_weights`): seg_label -- the flat int64 label tensor of the 3D
    store (raw nyu40 ids, as the script's pickle holds them) or a list of per-scene tensors, on the device -- counted into num_labels bins
    (ops.label_histogram, one launch per tensor into one histogram), then metric.label_log_weights at class_ids (the default is the
    script's VALID_CLASS_IDS; None: every bin).  -> (len(class_ids),) float32 NumPy array."""
    hist = None
    for t in ([seg_label] if torch.is_tensor(seg_label) else list(seg_label)):
        hist = ops.label_histogram(t, num_labels, out=hist)
    if hist is None:
        raise RuntimeError('label_weights_3d: no labels')
    return metric.label_log_weights(hist, class_ids)
