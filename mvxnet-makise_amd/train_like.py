"""A training loop with the call sequence of the reference's train.py (train.py:26-49 per-frame preparation, :51-180
loop, checkpoints and resume), running on this package's HIP modules.

    python train_like.py <dataroot> [-n EPOCHS] [-r LAST] [--steps K] [--mode module|fast] [--frames B] [--synthetic N]
                         [--augment [--gtdatabase DIR]] [--augment-geometry] [--extractor-weights FILE]
                         [--optimizer torch|hip [--clip-grad-norm X] [--lr-schedule constant|cosine --warmup-steps N --lr-min LR]]
                         [--loss voxel|focal [--focal-alpha A --focal-gamma G --focal-reg-weight W]]

What is the same as train.py: createDataset -> createAnchors / bbox3d2bev -> MVXNet, VoxelLoss, AdamW(lr 1e-3, eps) ->
per frame lidar2Img + (row, col) swap + group + classifyAnchors -> forward -> clsLoss (+ regLoss) -> backward -> step ->
running loss statistics -> per-epoch ``checkpoints/epoch{n}.pkl`` / ``epoch{n}_opt.pkl`` and ``-r`` resume.
The GT-paste augmentation of train.py:28 is there with ``--augment`` (modules/augment, on the GPU; ``--synthetic`` also writes
a synthetic gtdatabase; off by default); ``--augment-geometry`` adds VoxelNet's per-object noise, global scaling and rotation and
the y flip behind it or alone (modules/augment/Geometry.py).  The frozen image extractor runs on this package's own kernels with
``--extractor-weights FILE`` (a state dict with torchvision's key names, e.g. a checkpoint of the reference's train.py;
modules/imhead/Extractor.py): every frame's image then goes through it, after the GT paste when ``--augment`` is on.  Without
the flag the FPN maps are deterministic synthetic tensors per frame (or, in --mode module with torchvision installed, come
from torchvision).

``--optimizer hip`` replaces torch.optim.AdamW by the library's fused AdamW (modules/optim.py: one streaming pass over the flat
gradient bucket, the division by the frame count folded in), with global gradient-norm clipping (``--clip-grad-norm``), a guard
that skips a step with a non-finite gradient on the device, and a warm-up + cosine learning-rate schedule.  Checkpoints keep
torch.optim.AdamW's format: a run can resume with either optimizer from a checkpoint of the other.

``--loss focal`` (--mode fast only) replaces VoxelLoss by the focal loss of modules/voxelnet/FocalLoss.py: one library call for
all frames of a step on the logits of the heads; anchors between the two IoU thresholds are ignored.

``--direction`` (--mode fast --loss focal only) trains the heading as SECOND / PointPillars do: the model gets a two-way
direction classifier per anchor (``backbone.rpn.dir``), the angle is regressed through the sine of its residual, and the
decode of detect_like.py folds the yaw back with the classifier's bit.  ``--dir-weight`` / ``--dir-offset`` are FocalLoss's;
pass the same ``--dir-offset`` to detect_like.py / visualize_like.py (the checkpoint is the bare state dict).

``--iou-head`` (with ``--direction``; ``--iou-weight``, default 1.0) adds the IoU-aware confidence head of CIA-SSD / AFDetV2
(``backbone.rpn.iou``): one logit per anchor trained to predict the 3D IoU of the decoded box with its ground truth, which
detect_like.py multiplies into the score (``--iou-alpha`` there).

``--iou-loss`` (--mode fast --loss focal only; ``--iou-loss-weight``, default 1.0; with or without the two heads above) adds the
rotated 3D IoU regression loss ``1 - IoU3D`` of every positive to the regression loss, its analytic gradient flowing into the
seven regression columns (csrc/box_iou_loss.hip).  The loop prints the epoch's mean IoU of the positives.

--mode module : the reference's own interface, one frame at a time: ``model(voxel, img, idx, [calib], imsize)``.
--mode fast   : B frames per step through the frame-set executor (modules/frames.py: one launch per layer for all
                frames), RPN + VoxelLoss per frame (per-frame BatchNorm statistics, as B reference forwards), one AdamW
                step per B frames on the summed gradient / B; data-parallel over ranks when launched with torchrun.
"""
import argparse
import math
import os
import random
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dataroot', nargs='?', default=None)
    ap.add_argument('-n', '--numepochs', type=int, default=1)
    ap.add_argument('-r', '--resume', type=int, default=0, dest='lastiter')
    ap.add_argument('--steps', type=int, default=0, help='stop after this many optimizer steps (0 = whole epochs)')
    ap.add_argument('--mode', choices=['module', 'fast'], default='module')
    ap.add_argument('--frames', type=int, default=4, help='frames per step in --mode fast')
    ap.add_argument('--synthetic', type=int, default=0, help='write a synthetic KITTI tree with this many frames into dataroot first')
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--checkpoints', default='./checkpoints')
    ap.add_argument('--need-crop', action='store_true', help='read training/velodyne and crop on the GPU (cropdata.py on the fly)')
    ap.add_argument('--quiet', action='store_true')
    ap.add_argument('--prefetch', action='store_true',
                    help='--mode fast: prepare batch k+1 on a worker thread + stream (modules/data/Prefetch.py); off by default: with '
                         'the preparation on the GPU the loop already runs at the step time, and the thread costs more than it hides')
    ap.add_argument('--prefetch-depth', type=int, default=2)
    ap.add_argument('--prefetch-priority', type=int, default=-1, help='HIP stream priority of the loader stream (-1 high, 0 default)')
    ap.add_argument('--augment', action='store_true', help='GT-paste augmentation (train.py:28: up to 12 cars per frame)')
    ap.add_argument('--gtdatabase', default=None, help='root that holds training/gtdatabase (default: dataroot)')
    ap.add_argument('--augment-objects', type=int, default=200, help='objects of the synthetic gtdatabase (--synthetic --augment)')
    ap.add_argument('--augment-geometry', action='store_true',
                    help='geometric augmentation (VoxelNet 3.2: per-object noise, global scaling and rotation; plus the y flip), '
                         'with or without --augment')
    ap.add_argument('--extractor-weights', default=None,
                    help='state dict of the frozen ResNet50-FPN extractor (torchvision key names): images go through the HIP extractor')
    ap.add_argument('--optimizer', choices=['torch', 'hip'], default='torch',
                    help='hip: the fused AdamW of modules/optim.py (clipping, non-finite guard, schedule); same checkpoint format')
    ap.add_argument('--clip-grad-norm', type=float, default=0.0, help='--optimizer hip: clip the global gradient norm to this (0 = off)')
    ap.add_argument('--lr-schedule', choices=['constant', 'cosine'], default='constant', help='--optimizer hip: cosine = linear warm-up, then cosine')
    ap.add_argument('--warmup-steps', type=int, default=0)
    ap.add_argument('--lr-min', type=float, default=0.0)
    ap.add_argument('--loss', choices=['voxel', 'focal'], default='voxel',
                    help='voxel: the reference\'s VoxelLoss; focal: modules/voxelnet/FocalLoss.py on the logits of all frames of a '
                         'step in one call (--mode fast only)')
    ap.add_argument('--targets', choices=['reference', 'maxiou'], default='reference',
                    help='reference: the reference\'s classifyAnchors; maxiou: Calc.assignAnchorsFrames (thresholds 0.45 / 0.6 on the '
                         'best box of every anchor, plus the best anchor of every box)')
    ap.add_argument('--force-iou', type=float, default=0.1,
                    help='--targets maxiou: a box whose best IoU reaches this gets its best anchor as a positive (2 = thresholds only)')
    ap.add_argument('--ignore-dontcare', action='store_true',
                    help='--targets maxiou --mode fast: anchors whose centre projects into a DontCare rectangle leave the classification loss')
    ap.add_argument('--ignore-classes', nargs='+', default=[], metavar='CLASS',
                    help='--targets maxiou --mode fast: anchors covered by a box of these classes (Van, Truck, Tram ...) leave the '
                         'classification loss')
    ap.add_argument('--ignore-ioa', type=float, default=0.5,
                    help='--ignore-classes: share of the ANCHOR\'s area that such a box must cover, in (0, 1] (0.5 is a design choice, '
                         'not a measured optimum)')
    ap.add_argument('--min-gt-points', type=int, default=0,
                    help='--targets maxiou --mode fast: a Car with fewer points than this, counted after crop and augmentation, gives no '
                         'positive; its anchors are ignored (0 = off: a design choice, not a measured optimum)')
    ap.add_argument('--focal-alpha', type=float, default=0.25)
    ap.add_argument('--focal-gamma', type=float, default=2.0)
    ap.add_argument('--focal-reg-weight', type=float, default=2.0)
    ap.add_argument('--direction', action='store_true',
                    help='--mode fast --loss focal: a direction classifier per anchor and the sine angle loss (MVXNet(direction=True), '
                         'FocalLoss(direction=True))')
    ap.add_argument('--dir-weight', type=float, default=0.2, help='--direction: weight of the direction loss (SECOND\'s value)')
    ap.add_argument('--dir-offset', type=float, default=math.pi / 4,
                    help='--direction: yaw at which the direction bit flips (SECOND\'s pi/4); detect_like.py takes the same value')
    ap.add_argument('--iou-head', action='store_true',
                    help='--direction: an IoU-aware confidence logit per anchor (MVXNet(direction=True, iou=True), '
                         'FocalLoss(direction=True, iou=True)); detect_like.py rectifies the scores with it')
    ap.add_argument('--iou-weight', type=float, default=1.0,
                    help='--iou-head: weight of the IoU loss (a design choice, not an optimum measured here)')
    ap.add_argument('--iou-loss', action='store_true',
                    help='--mode fast --loss focal: add the rotated 3D IoU regression loss 1 - IoU3D, with its analytic gradient, to '
                         'the regression loss (FocalLoss(iou_loss=True)); with or without --direction / --iou-head')
    ap.add_argument('--iou-loss-weight', type=float, default=1.0,
                    help='--iou-loss: weight of the term (a design choice, not an optimum measured here)')
    ap.add_argument('--bn-track', action='store_true',
                    help='--mode fast: running BatchNorm statistics (config.yml bntrack: True does the same): the checkpoints carry '
                         'running_mean / running_var / num_batches_tracked, detect_like.py then runs the model in eval mode')
    ap.add_argument('--bn-momentum', type=float, default=0.1, help='--bn-track: momentum of the running statistics (torch\'s default)')
    args = ap.parse_args(argv)
    if args.bn_track and args.mode != 'fast':
        ap.error('--bn-track needs --mode fast: the running statistics are kept on the frame-set path')
    if not 0.0 <= args.bn_momentum <= 1.0:
        ap.error('--bn-momentum must lie in 0..1')
    if args.iou_head and not args.direction:
        ap.error('--iou-head needs --direction: the IoU logits take the two pad columns of the direction model\'s head rows')
    if args.iou_weight < 0:
        ap.error('--iou-weight must not be negative')
    if args.iou_loss and (args.mode != 'fast' or args.loss != 'focal'):
        ap.error('--iou-loss needs --mode fast --loss focal: the term is computed on the frame-set heads behind the focal loss')
    if not args.iou_loss_weight >= 0:
        ap.error('--iou-loss-weight must not be negative')
    if args.direction and (args.mode != 'fast' or args.loss != 'focal'):
        ap.error('--direction needs --mode fast --loss focal: the direction head is trained by the focal loss of the frame-set '
                 'heads only')
    if args.loss == 'focal' and args.mode == 'module':
        ap.error('--loss focal needs --mode fast: the focal loss reads the logits of the frame-set heads, --mode module hands the '
                 'criterion probabilities')
    if args.force_iou <= 0:
        ap.error('--force-iou must be positive (2 = thresholds only)')
    args.ignore = bool(args.ignore_dontcare or args.ignore_classes or args.min_gt_points)
    if (args.ignore or args.ignore_ioa != 0.5) and args.targets != 'maxiou':
        ap.error('--ignore-dontcare / --ignore-classes / --ignore-ioa / --min-gt-points need --targets maxiou: the ignore pass '
                 'rewrites the lists of the max-IoU assigner')
    if args.ignore and args.mode != 'fast':
        ap.error('--ignore-dontcare / --ignore-classes / --min-gt-points need --mode fast: the pass runs on the frame set of a step')
    if not 0.0 < args.ignore_ioa <= 1.0:
        ap.error('--ignore-ioa must lie in (0, 1]')
    if args.min_gt_points < 0:
        ap.error('--min-gt-points must not be negative')
    return args


def check_optimizer_args(args):
    """Flags that only the HIP optimizer implements must not be silently ignored with the torch one."""
    if args.optimizer == 'torch':
        if args.clip_grad_norm:
            raise SystemExit('--clip-grad-norm needs --optimizer hip (the torch optimizer path does not clip)')
        if args.lr_schedule != 'constant' or args.warmup_steps or args.lr_min:
            raise SystemExit('--lr-schedule / --warmup-steps / --lr-min need --optimizer hip (the torch optimizer path trains at a constant 1e-3)')
    if args.clip_grad_norm < 0 or args.warmup_steps < 0 or args.lr_min < 0:
        raise SystemExit('--clip-grad-norm, --warmup-steps and --lr-min must not be negative')


def fpn_maps_for(name, dev):
    """Stand-in for the frozen extractor when torchvision is absent: deterministic maps per frame name, generated on the
    device (47 MB per frame: drawing them on the host would make the stand-in the slowest part of the loop)."""
    g = torch.Generator(device=dev).manual_seed(3000 + int(name))
    return [torch.randn((1, 256, h, w), generator=g, device=dev).contiguous(memory_format=torch.channels_last)
            for h, w in ((104, 336), (52, 168), (26, 84))]


def extractor_fpn_fn(extractor, images_by_name):
    """``fpn_fn`` of the real extractor: the frame's camera image (H, W, 3) u8 -> its three FPN maps."""
    def fpn_fn(name, dev):
        img = torch.from_numpy(np.ascontiguousarray(images_by_name[name], dtype=np.uint8)).to(dev)
        return extractor.extract_frames(img[None])[0]
    return fpn_fn


def have_torchvision():
    try:
        import torchvision  # noqa: F401
        return True
    except ImportError:
        return False


def cputask(data, anchorBevs, cfg, gtwithinfo=None, geometry=None, assigner=None):
    """train.py:26-49: (GT-paste augmentation when ``gtwithinfo`` is given,) projection, (row, col) swap, voxelization,
    target assignment.  ``geometry`` = {'params', 'rng'}: the geometric augmentation between the projection and the grouping,
    so that every point keeps the pixel it was seen at.  ``assigner`` (``frames -> lists``, --targets maxiou) takes the place of
    classifyAnchors, as one frame."""
    from modules.Calc import classifyAnchors
    from modules.data import Preprocessing as pre
    from modules.utils import lidar2Img
    pcd, img, bbox2d, bbox3d, bev, calib = data
    augpcd, augcalib = [], []
    if gtwithinfo is not None:
        from modules.augment.Augment import augmentTargetClasses
        augpcd, augcalib, img, bbox3d, bev = augmentTargetClasses(pcd, img, bbox2d, bbox3d, bev, gtwithinfo, ['Car'], [12])
        bbox3d, bev = bbox3d['Car'], bev['Car']
    pcd_t = torch.Tensor(pcd)
    proj = lidar2Img(pcd_t, calib, True)[:, [1, 0]]
    pcd6 = torch.concat([pcd_t, proj.cpu()], dim=1).numpy()
    if augpcd:
        pcdxy = [pcd6]
        for ap_, ac in zip(augpcd, augcalib):
            pcdxy.append(np.concatenate([ap_, lidar2Img(ap_, ac, True)[:, ::-1]], axis=1))
        pcd6 = np.concatenate(pcdxy, axis=0).astype(np.float32)          # train.py:125 casts the voxels to float32
    if geometry is not None:
        from modules.augment.Geometry import augmentGeometry
        pcd6, bbox3d, bev = augmentGeometry(pcd6, bbox3d, params=geometry.get('params'), rng=geometry['rng'])
    voxel, idx = pre.group(pcd6, cfg.velorange, cfg.voxelsize, cfg.samplenum)
    if bev is not None and bev.shape[0] != 0:
        if assigner is not None:
            pi, ni, gi = assigner([(bev, bbox3d[:, [0, 1]])])[0]
        else:
            pi, ni, gi = classifyAnchors(bev, bbox3d[:, [0, 1]], anchorBevs, cfg.velorange, 0.45, 0.6)
    else:
        pi, ni, gi = None, None, None
    return voxel, idx, img, bbox3d, bev, pi, ni, gi, calib


def fast_chunks(n_frames, frames_per_rank, world):
    """[lo, hi) frame ranges of the global steps of one epoch in --mode fast: the same list on every rank."""
    stride = frames_per_rank * world
    return [(lo, min(n_frames, lo + stride)) for lo in range(0, n_frames, stride)]


def train(args):
    """The training loop; ``--bn-track`` switches ``bntrack`` on for its duration (the configuration is restored on return)."""
    import modules.config as cfg
    old = cfg.config.get('bntrack', False)
    if getattr(args, 'bn_track', False):
        cfg.config['bntrack'] = True
    try:
        return _train(args)
    finally:
        cfg.config['bntrack'] = old


def _train(args):
    check_optimizer_args(args)
    import modules.config as cfg
    from modules import bn_running as bnr
    from modules import parallel
    from modules.Calc import bbox3d2bev
    from modules.data import Load as load, Preprocessing as pre
    from modules.voxelnet import VoxelLoss
    from MVXNet import MVXNet

    rank, world, local = parallel.init_from_env()
    device = torch.device('cuda', local % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(device)
    say = (lambda *a, **k: None) if (args.quiet or rank != 0) else print

    if args.synthetic:
        from modules.data import Synthetic
        if rank == 0:
            Synthetic.write_kitti_tree(args.dataroot, list(range(args.synthetic)), points=args.points)
            if args.augment and args.gtdatabase is None:
                Synthetic.write_gt_database(args.dataroot, args.augment_objects)
        if world > 1:
            torch.distributed.barrier()
    with open(os.path.join(args.dataroot, 'ImageSets/train.txt'), 'r') as f:
        trainSet = f.read().splitlines()
    t_ds = time.perf_counter()
    trainDataSet = load.createDataset(trainSet, needCrop=args.need_crop, root=args.dataroot)
    dataset_s = time.perf_counter() - t_ds           # file I/O: the whole split is read into RAM first, like train.py:53-57
    names = {id(d): n for d, n in zip(trainDataSet, trainSet)}
    gtwithinfo = aug = None
    if args.augment:
        from modules.augment.LoadGT import getAllGT, GTDatabase
        gtwithinfo = getAllGT(['Car'], root=args.gtdatabase or args.dataroot)          # train.py:57
        db = GTDatabase.from_gts(gtwithinfo['Car'], device)
        # --mode fast draws with a Generator: the reference-order draw permutes the whole database once per slot
        aug = {'db': db, 'lim': 12, 'rng': np.random.default_rng(rank)}
    geo = None
    if args.augment_geometry:
        from modules.augment.Geometry import GeomParams
        geo = {'params': GeomParams(), 'rng': np.random.default_rng([rank, 1])}          # per rank, apart from the paste's stream
    if args.augment:
        say('gtdatabase: %d objects, %.1f MB resident, %d points dropped at load' % (db.n, db.nbytes() / 1e6, db.dropped_points))

    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    anchorBevs = bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(device).contiguous()
    assigner, assign_stats = None, {'boxes': 0, 'forced_only': 0, 'none': 0}
    if args.targets == 'maxiou':
        from modules.Calc import assignAnchorsFrames

        def assigner(frames, ignore=None):
            info = {}
            lists = assignAnchorsFrames(frames, anchorBevs, 0.45, 0.6, args.force_iou, info=info, ignore=ignore)
            assign_stats['boxes'] += sum(b.numel() for b in info['gt_best'] if b is not None)
            assign_stats['forced_only'] += info['forced_only']
            assign_stats['none'] += info['none']
            if ignore is not None:
                ignore_stats[:] = [a + b for a, b in zip(ignore_stats, info['ignore_stats'])]
            return lists
    ign, ignore_stats = None, [0, 0, 0, 0]
    if args.ignore:
        rows = load.readIgnoreLabels(trainSet, root=args.dataroot, classes=tuple(args.ignore_classes))
        ign_labels = dict(zip(trainSet, rows))
        ign = {'anchors': anchors.reshape(anchors.shape[:2] + (-1, 7)), 'dontcare': args.ignore_dontcare, 'ioa': args.ignore_ioa,
               'min_points': args.min_gt_points, 'labels_of': lambda name: ign_labels[name]}
        say('ignore regions: %d DontCare rectangle(s)%s, %d box(es) of %s, Cars below %d point(s)'
            % (sum(r.shape[0] for r, _ in rows), '' if args.ignore_dontcare else ' (not used)', sum(b.shape[0] for _, b in rows),
               '/'.join(args.ignore_classes) or 'no class', args.min_gt_points))
    torch.manual_seed(0)
    tracked = bool(cfg.config.get('bntrack', False))
    if tracked and args.mode != 'fast':
        raise SystemExit('bntrack needs --mode fast: the running BatchNorm statistics are kept on the frame-set path')
    if args.iou_head:
        model = MVXNet(direction=True, iou=True).to(device)
    else:
        model = (MVXNet(direction=True) if args.direction else MVXNet()).to(device)
    if tracked:
        # every rank folds its own frames into its own buffers and rank 0's are saved: no buffer all-reduce (modules/parallel.py)
        bnr.set_momentum(model, getattr(args, 'bn_momentum', 0.1))
        say('bntrack: running BatchNorm statistics, momentum %g' % getattr(args, 'bn_momentum', 0.1))
    if args.loss == 'focal':
        from modules.voxelnet.FocalLoss import FocalLoss
        box = dict(iou_loss=True, iou_loss_weight=args.iou_loss_weight) if args.iou_loss else {}
        if args.iou_head:
            criterion = FocalLoss(alpha=args.focal_alpha, gamma=args.focal_gamma, reg_weight=args.focal_reg_weight, direction=True,
                                  dir_weight=args.dir_weight, dir_offset=args.dir_offset, iou=True, iou_weight=args.iou_weight, **box)
        elif args.direction:
            criterion = FocalLoss(alpha=args.focal_alpha, gamma=args.focal_gamma, reg_weight=args.focal_reg_weight, direction=True,
                                  dir_weight=args.dir_weight, dir_offset=args.dir_offset, **box)
        else:
            criterion = FocalLoss(alpha=args.focal_alpha, gamma=args.focal_gamma, reg_weight=args.focal_reg_weight, **box)
        say('criterion: FocalLoss(alpha=%g, gamma=%g, cls_weight=%g, reg_weight=%g)'
            % (criterion.alpha, criterion.gamma, criterion.cls_weight, criterion.reg_weight))
        if args.direction:
            say('direction head: dir_weight=%g, dir_offset=%g, sine angle loss' % (criterion.dir_weight, criterion.dir_offset))
        if args.iou_head:
            say('IoU head: iou_weight=%g' % criterion.iou_weight)
        if args.iou_loss:
            say('rotated IoU regression loss: iou_loss_weight=%g, added to the regression loss' % criterion.iou_loss_weight)
    else:
        criterion = VoxelLoss()
        say('criterion: VoxelLoss(a=%g, b=%g)' % (criterion.a, criterion.b))
    params =[p for p in model.parameters() if p.requires_grad]
    # train.py:64; on the GPU as one fused multi-tensor kernel per step (same update, ~10 launches fewer; bench.py has the numbers)
    hip_opt = args.optimizer == 'hip'
    bucket = parallel.GradBucket(params, late=[model.head.fusion.fcn1.fc.weight]) if args.mode == 'fast' else None
    if hip_opt:
        from modules import optim
        # --mode fast: on the step's own bucket; --mode module: on a bucket the optimizer makes (autograd then accumulates into it)
        opt = optim.AdamW(params, lr=0.001, eps=cfg.eps, max_norm=args.clip_grad_norm, bucket=bucket)
    else:
        opt = torch.optim.AdamW(params, lr=0.001, eps=cfg.eps, fused=(device.type == 'cuda'))
    anchors = anchors.to(device)
    imsize = torch.Tensor(cfg.imsize).to(device)
    os.makedirs(args.checkpoints, exist_ok=True)
    if args.lastiter > 0:
        if bnr.load_state(model, torch.load(os.path.join(args.checkpoints, 'epoch%d.pkl' % args.lastiter), map_location=device)):
            say('bntrack: epoch%d.pkl holds no running statistics: the buffers start at mean 0, variance 1' % args.lastiter)
        opt.load_state_dict(torch.load(os.path.join(args.checkpoints, 'epoch%d_opt.pkl' % args.lastiter), map_location=device))
    tv = have_torchvision()
    fpn_fn = fpn_maps_for
    if args.extractor_weights:
        if args.prefetch and aug is not None:
            raise SystemExit('--extractor-weights with --augment runs the extractor after the paste, inside the step: drop --prefetch')
        model.head.extractor.load_weights(args.extractor_weights).to(device)
        fpn_fn = extractor_fpn_fn(model.head.extractor, {n: d[1] for d, n in zip(trainDataSet, trainSet)})
        if aug is not None:
            aug['extractor'] = model.head.extractor
        tv = True                                  # --mode module: the image itself goes to the model

    forwardTime = lossTime = backwardTime = 0.0
    steps_done, losses, loop_stats = 0, [], []
    if args.mode == 'module':
        steps_per_epoch = len(trainDataSet)
    else:
        steps_per_epoch = len(fast_chunks(len(trainDataSet), args.frames, world))
    # position in the schedule: host calls of step(), skipped ones included; a resumed run continues where epoch `lastiter` ended
    sched_k = args.lastiter * steps_per_epoch
    sched_total = (args.lastiter + args.numepochs) * steps_per_epoch

    def next_lr():
        nonlocal sched_k
        lr = optim.lr_at(sched_k, 0.001, args.lr_schedule, args.warmup_steps, sched_total, args.lr_min)
        sched_k += 1
        return lr

    def report_optimizer(n):
        if hip_opt:                               # one host read per epoch
            d = opt.diagnostics()
            say('Epoch%d optimizer: step %d, last gradient norm %.6g (clip coefficient %.4g), %d step(s) skipped for a non-finite gradient'
                % (n, d['step'], d['norm'], d['coef'], d['skipped']))

    for epoch in range(args.numepochs):
        random.Random(epoch + args.lastiter).shuffle(trainDataSet)
        mine = trainDataSet
        clsLossSum = regLossSum = dirLossSum = iouLossSum = 0.0
        clsCnt = regCnt = dirCnt = iouCnt = 0
        boxIouSum, boxIouCnt = 0.0, 0              # --iou-loss: mean IoU of the positives, per frame that has one
        if args.mode == 'module':
            for i, data in enumerate(mine):
                voxel, idx, img, gt, gtbev, pi, ni, gi, calibCpu = cputask(data, anchorBevs, cfg, gtwithinfo, geo, assigner)
                calib = {k: torch.Tensor(calibCpu[k]).to(device) for k in calibCpu}
                idx4 = np.concatenate([np.zeros((idx.shape[0], 1)), idx], axis=1)
                opt.zero_grad()
                st = time.perf_counter()
                voxel_t = torch.Tensor(voxel[None, :]).to(device)
                idx_t = torch.LongTensor(idx4).to(device)
                if tv:
                    x = (torch.Tensor(img.copy()).to(device).permute(2, 0, 1) / 255)[None]
                else:
                    x = fpn_maps_for(names[id(data)], device)
                score, reg = model(voxel_t, x, idx_t, [calib], imsize)
                score = score.squeeze(dim=0).permute(1, 2, 0)
                reg = reg.squeeze(dim=0).permute(1, 2, 0)
                forwardTime += time.perf_counter() - st
                st = time.perf_counter()
                clsLoss, regLoss = criterion(pi, ni, gi, gt.to(device) if gt is not None else None, score, reg, anchors, 2)
                loss = clsLoss if regLoss is None else clsLoss + regLoss
                lossTime += time.perf_counter() - st
                st = time.perf_counter()
                loss.backward()
                if hip_opt:
                    opt.step(lr=next_lr())
                else:
                    opt.step()
                backwardTime += time.perf_counter() - st
                c = float(clsLoss.detach())
                if c == c:
                    clsLossSum += c
                    clsCnt += 1
                if regLoss is not None:
                    regLossSum += float(regLoss.detach())
                    regCnt += 1
                losses.append(float(loss.detach()))
                steps_done += 1
                if (i + 1) % 50 == 0 or i + 1 == len(mine):
                    say('Epoch%d %d/%d  average classification loss %.6f, average regression loss %.6f'
                        % (epoch + args.lastiter + 1, i + 1, len(mine), clsLossSum / max(1, clsCnt), regLossSum / max(1, regCnt)))
                if args.steps and steps_done >= args.steps:
                    break
        else:
            from modules import pipeline as pl
            B = args.frames
            # ONE step count for every rank, derived from the global length (ranks that ran different numbers of steps would
            # issue different collective sequences): global step g covers frames [g*B*W, (g+1)*B*W) of the shuffled epoch,
            # rank r takes every W-th of them.  The last chunk may be short -- the reference trains on every frame
            # (train.py:110) -- so a rank may get fewer than B frames, or none: it still takes part in the all-reduce with
            # a zero gradient, and the divisor is the number of frames that contributed on all ranks.
            chunks = fast_chunks(len(trainDataSet), B, world)
            groups = [trainDataSet[lo + rank:hi:world] for lo, hi in chunks]
            cap = max(args.points, max(d[0].shape[0] for d in trainDataSet))
            if aug is not None:
                cap += aug['lim'] * aug['db'].max_points                 # room for the pasted objects
            if not args.prefetch:
                def batches():
                    for group in groups:
                        if not group:
                            yield None, None
                        else:
                            gnames = [names[id(d)] for d in group]
                            ig = None if ign is None else dict(ign, labels=[ign_labels[n] for n in gnames])
                            yield pl.batch_from_dataset(group, gnames, device, anchorBevs, fpn_fn, cap_points=cap,
                                                        augment=aug, geometry=geo, assigner=assigner, ignore=ig)
                loader = batches()
            else:
                # batch k+1 is prepared by a worker thread on its own stream while step k runs (the reference overlaps its CPU
                # preparation with a process pool, train.py:185-187)
                from modules.data.Prefetch import PrefetchLoader
                loader = PrefetchLoader(groups, lambda d: names[id(d)], device, anchorBevs, fpn_fn, cap,
                                        depth=args.prefetch_depth, priority=args.prefetch_priority, augment=aug, geometry=geo,
                                        assigner=assigner, ignore=ign)
            pending = None                       # the losses of a step are read one step later: the host never waits for
                                                  # the step it has just enqueued

            def account(p):
                nonlocal clsLossSum, clsCnt, regLossSum, regCnt, dirLossSum, dirCnt, iouLossSum, iouCnt, boxIouSum, boxIouCnt
                if p is None:
                    return
                pl.read_losses(p)
                if p.get('box_iou') is not None:          # read with the losses, a step later
                    for (_, mean_q), hr in zip(p['box_iou'].tolist(), p['has_reg']):
                        if hr:
                            boxIouSum += mean_q
                            boxIouCnt += 1
                losses.extend(p['loss'])
                clsLossSum += sum(p['cls'])
                clsCnt += len(p['cls'])
                regLossSum += sum(p['reg'])
                regCnt += len(p['reg'])
                dirLossSum += sum(p.get('dir', ()))
                dirCnt += len(p.get('dir', ()))
                iouLossSum += sum(p.get('iou', ()))
                iouCnt += len(p.get('iou', ()))

            t_epoch = time.perf_counter()
            frames_epoch = 0
            for gstep, ((lo, hi), (batch, targets)) in enumerate(zip(chunks, loader)):
                st = time.perf_counter()
                bucket.zero()
                used = 0
                out = None
                if batch is not None:
                    out = pl.train_step_full(model, batch, targets, criterion, anchors, cfg.imsize, read=False)
                    used = len(out['live'])
                    if args.iou_loss and 'losses_dev' in out:
                        out['box_iou'] = criterion.last_box_iou
                    if used < batch.n_frames:
                        say('Epoch%d step %d: %d frame(s) without a voxel skipped' % (epoch + args.lastiter + 1, gstep, batch.n_frames - used))
                forwardTime += time.perf_counter() - st
                # this rank's frame count rides in the bucket's count slot: the global divisor is applied on the device, with no
                # second collective and no host read (a blocking count exchange undid read=False)
                if hip_opt:
                    # the sum and the global count stay in the buffer: the update applies 1 / max(count, 1) as it reads the gradient
                    bucket.all_reduce_mean(frames_local=used, divide=False)
                    opt.step(lr=next_lr(), count=bucket.count_slot())
                else:
                    bucket.all_reduce_mean(frames_local=used)
                    opt.step()
                account(pending)
                pending = out
                frames_epoch += hi - lo
                steps_done += 1
                say('Epoch%d %d/%d  average classification loss %.6f, average regression loss %.6f%s%s'
                    % (epoch + args.lastiter + 1, hi, len(trainDataSet), clsLossSum / max(1, clsCnt), regLossSum / max(1, regCnt),
                       ', average direction loss %.6f' % (dirLossSum / max(1, dirCnt)) if args.direction else '',
                       ', average IoU loss %.6f' % (iouLossSum / max(1, iouCnt)) if args.iou_head else ''))
                if args.steps and steps_done >= args.steps:
                    break
            account(pending)
            if hasattr(loader, 'close'):
                loader.close()
            torch.cuda.synchronize(device)
            loop_s = time.perf_counter() - t_epoch
            loop_stats.append({'epoch': epoch + args.lastiter + 1, 'frames': frames_epoch, 'seconds': loop_s,
                               'frames_per_s': frames_epoch / loop_s if loop_s > 0 else 0.0,
                               'loader': dict(getattr(loader, 'stats', {}))})
            say('Epoch%d: %d frames in %.2f s = %.1f frames/s (all ranks, %s)'
                % (epoch + args.lastiter + 1, frames_epoch, loop_s, frames_epoch / max(loop_s, 1e-9),
                   'prefetch thread' if args.prefetch else 'batches prepared inside the step'))
            if args.iou_loss:
                say('Epoch%d: mean 3D IoU of the positives with their boxes %.4f (over %d frame(s) with a positive)'
                    % (epoch + args.lastiter + 1, boxIouSum / max(1, boxIouCnt), boxIouCnt))
        if assigner is not None:
            say('Epoch%d targets: %d boxes, %d with only a forced positive, %d with none'
                % (epoch + args.lastiter + 1, assign_stats['boxes'], assign_stats['forced_only'], assign_stats['none']))
            assign_stats.update(boxes=0, forced_only=0, none=0)
        if ign is not None:
            say('Epoch%d ignored: %d positive(s) demoted, %d anchor(s) by a DontCare rectangle, %d by a look-alike box, %d sparse box(es)'
                % ((epoch + args.lastiter + 1,) + tuple(ignore_stats)))
            ignore_stats[:] = [0, 0, 0, 0]
        report_optimizer(epoch + args.lastiter + 1)
        if rank == 0:
            n = epoch + args.lastiter + 1
            torch.save(model.state_dict(), os.path.join(args.checkpoints, 'epoch%d.pkl' % n))
            torch.save(opt.state_dict(), os.path.join(args.checkpoints, 'epoch%d_opt.pkl' % n))
        if args.steps and steps_done >= args.steps:
            break
    if args.mode == 'fast':
        parallel.assert_replicas_in_sync(params)
    say('forward %.2f s, loss %.2f s, backward %.2f s' % (forwardTime, lossTime, backwardTime))
    return {'losses': losses, 'steps': steps_done, 'model': model, 'opt': opt, 'loop': loop_stats, 'dataset_s': dataset_s,
            'dataset_frames': len(trainDataSet)}


if __name__ == '__main__':
    a = parse_args()
    if a.dataroot is None:
        raise SystemExit('usage: python train_like.py <dataroot> [--synthetic N] ...')
    sys.argv = sys.argv[:1]              # modules.config parses argv at import (reference modules/config/Parser.py:12)
    train(a)
