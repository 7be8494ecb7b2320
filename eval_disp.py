#!/usr/bin/env python3
"""Batched depth evaluation on the KITTI Eigen split / NYU: the command line of test_disp.py plus three flags,

    python3 eval_disp.py --pretrained-dispnet CKPT --network disp_vgg_BN --dataset-dir KITTI_RAW \
        --dataset-list kitti_eval/test_files_eigen.txt --eval-batch 32 --readers 16

--eval-batch N   N images per eval-mode forward; cubic-spline zoom to each ground-truth size, clip, mask, median / x5.4 scale and the
                 seven metrics run on the device (supervised_dispnet_amd/evaluation.py).  0 (the default) hands
                 the whole run to test_disp.py's per-image host chain.
--device-resize  with --eval-batch on KITTI: the frames are uploaded as they are and byte-scaled, resized and normalised on the device
                 (dn_imresize_u8; bit for bit the host resize).  NYU and --no-resize keep the host path.
--readers N      host threads (default 4, at most 16) that read framework[j] -- image, velodyne projection, mask -- ahead of the GPU.
--protocol P     reference (the default): test_disp.py's chain, as above.  monodepth2: the chain of monodepth2's evaluate_depth.py, the one
                 its published tables come from -- the disparity is resized bilinearly to the ground-truth size
                 and inverted, the median ratio (--mono / --unsupervised) or x5.4 (--stereo) is applied FIRST and the result clamped to
                 [1e-3, 80] LAST, and the median and spread of the ratios are printed.  With --eval-batch on the device
                 (csrc/dn_eval_mono2.hip); without, per image in numpy (evaluation.mono2_evaluate_sample).  KITTI only; no SID network,
                 no --error.
--post-process   with --protocol monodepth2: the prediction is averaged with that of the mirrored frame (one forward at 2N), the "+pp"
                 rows of monodepth2's tables.

The printed lines, the returned mean errors and predictions.npy are those of test_disp.py (--protocol monodepth2 keeps the layout, puts
its own numbers in and adds the line on the scaling ratios in the median mode; predictions.npy stays 1 / disp at network resolution).  --error (the worst-300-pixel report) stays
on the per-image host chain and refuses --eval-batch.  The PoseNet-scaled evaluation (--pretrained-posenet) and the --pic comparison
plots are outside this path, as they are outside test_disp.py's.

Why a script of its own: test_disp.py carries the reference's command line and is kept exactly as it is (existing files named test_*.py are
yardsticks in this repository and a feature leaves them alone), so these flags cannot live there.  With --eval-batch this script therefore repeats
test_disp.main's set-up around its own loop; tests/test_gpu_eval_device.py holds the two mains to the same printed lines and results.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import test_disp  # noqa: E402  (the reference's command line: parser, network construction, the per-image chain)
from supervised_dispnet_amd.evaluation import check_protocol, prefetched  # noqa: E402

MAX_READERS = 16


def add_flags(p):
    p.add_argument("--eval-batch", default=0, type=int, metavar="N",
                   help="images per forward with zoom, mask, scale and metrics on the device; 0: test_disp.py's per-image host chain")
    p.add_argument("--device-resize", action="store_true",
                   help="with --eval-batch on KITTI: upload the raw frames and resize them on the device (dn_imresize_u8) instead of on the host")
    p.add_argument("--readers", default=4, type=int, metavar="N", help="host threads that read ahead for --eval-batch (at most 16)")
    p.add_argument("--protocol", default="reference", choices=["reference", "monodepth2"],
                   help="reference: test_disp.py's chain; monodepth2: evaluate_depth.py's (bilinear resize of the disparity, scale, then clamp)")
    p.add_argument("--post-process", action="store_true",
                   help="with --protocol monodepth2: average the prediction with that of the mirrored frame (the '+pp' rows of its tables)")
    return p


def build_parser():
    p = add_flags(test_disp.build_parser())
    p.allow_abbrev = False            # flags are spelled out here, so that host_chain_argv finds this script's own by the same rule
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.eval_batch < 0:
        raise SystemExit("eval_disp.py: --eval-batch must be >= 0")
    if args.device_resize and not args.eval_batch:
        raise SystemExit("eval_disp.py: --device-resize belongs to the batched chain; add --eval-batch N")
    if args.eval_batch and args.error:
        raise SystemExit("eval_disp.py: --error (the worst-300-pixel report) runs on the per-image host chain; drop --eval-batch")
    if args.protocol == "monodepth2" and args.error:
        raise SystemExit("eval_disp.py: --error (the worst-300-pixel report) belongs to the reference's chain; drop --protocol monodepth2")
    try:
        check_protocol(args.protocol, args.post_process, args.gt_type, args.network)
    except ValueError as e:
        raise SystemExit("eval_disp.py: {}".format(e))
    args.readers = max(1, min(MAX_READERS, args.readers))
    return args


def host_chain_argv(argv):
    """argv without the flags this script adds (and their values): what test_disp.main takes.  argparse itself picks them out."""
    import argparse
    return add_flags(argparse.ArgumentParser(add_help=False, allow_abbrev=False)).parse_known_args(list(argv))[1]


def evaluate_batched(args, disp_net, framework, device, min_depth, max_depth):
    """-> (errors float32 [7, n], predictions [n, h, w] with --output-dir, else None, the scale of every image float32 [n]) through the
    DeviceEvaluator, --eval-batch images at a time, while --readers threads read ahead."""
    from supervised_dispnet_amd.evaluation import DeviceEvaluator
    evaluator = DeviceEvaluator(args, disp_net, device, min_depth, max_depth)
    n = len(framework)
    errors, ratios = np.zeros((7, n), np.float32), np.zeros(n, np.float32)
    predictions, batch = None, []
    for j, sample in enumerate(prefetched(framework, n, args.readers, 2 * args.eval_batch + args.readers)):
        batch.append(sample)
        if len(batch) == args.eval_batch or j == n - 1:
            j0 = j + 1 - len(batch)
            errs, depths = evaluator.evaluate(batch)
            errors[:, j0:j + 1] = errs
            ratios[j0:j + 1] = evaluator.scales
            if args.output_dir is not None:
                if predictions is None:
                    predictions = np.zeros((n,) + depths[0].shape)
                predictions[j0:j + 1] = np.stack(depths)
            batch = []
    return errors, predictions, ratios


def evaluate_per_image(args, disp_net, framework, device, min_depth, max_depth):
    """The same three results from the per-image host chain of --protocol monodepth2 (evaluation.mono2_evaluate_sample): what runs
    without --eval-batch, since test_disp.main knows its own chain only."""
    from supervised_dispnet_amd.evaluation import mono2_evaluate_sample
    n = len(framework)
    errors, ratios = np.zeros((7, n), np.float32), np.zeros(n, np.float32)
    predictions = None
    for j in range(n):
        errors[:, j], ratios[j], depth = mono2_evaluate_sample(args, disp_net, framework[j], device, min_depth, max_depth, args.post_process)
        if args.output_dir is not None:
            if predictions is None:
                predictions = np.zeros((n,) + depth.shape)
            predictions[j] = depth
    return errors, predictions, ratios


@torch.no_grad()
def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if not args.eval_batch and args.protocol == "reference":
        return test_disp.main(host_chain_argv(argv))
    # the set-up of test_disp.main, then the batched loop (or, under --protocol monodepth2 without --eval-batch, its per-image host chain)
    if not torch.cuda.is_available():
        raise SystemExit("eval_disp.py drives the MI355X HIP path; no GPU is visible (there is no CPU fallback)")
    device = torch.device("cuda")
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    import supervised_dispnet_amd.models as models
    import supervised_dispnet_amd.networks as networks
    import supervised_dispnet_amd.utils as U
    from supervised_dispnet_amd import engine, kitti_eval as KE
    if args.compute is not None:
        engine.set_compute(args.compute)
    if args.gt_type not in ("KITTI", "NYU"):
        raise ValueError("gt-type '{}' is outside this path (KITTI and NYU are supported)".format(args.gt_type))
    if args.pretrained_posenet is not None:
        raise ValueError("PoseNet-scaled evaluation is outside this path; omit --pretrained-posenet")
    disp_net = test_disp.create_disp_net(args, models, networks, device, U)
    if not (args.mono or args.stereo):
        disp_net.load_state_dict(torch.load(args.pretrained_dispnet, map_location=device)["state_dict"])
    disp_net.eval()
    print("no PoseNet specified, scale_factor will be determined by median ratio, which is kiiinda cheating "
          "(but consistent with original paper)")
    if args.gt_type == "KITTI":
        min_depth, max_depth = 1e-3, 80
        if args.dataset_list is not None:
            with open(args.dataset_list) as f:
                test_files = f.read().splitlines()
        else:
            test_files = sorted(n for n in os.listdir(args.dataset_dir) if n.split(".")[-1] in args.img_exts)
        framework = KE.KittiTestFramework(args.dataset_dir, test_files, min_depth=min_depth, max_depth=max_depth, keep_u8=args.device_resize)
    else:
        min_depth, max_depth = 1e-3, 10
        framework = KE.NyuTestFramework(args.dataset_dir, min_depth=min_depth, max_depth=max_depth)
    print("{} files to test".format(len(framework)))
    run = evaluate_batched if args.eval_batch else evaluate_per_image
    errors, predictions, ratios = run(args, disp_net, framework, device, min_depth, max_depth)
    mean_errors = errors.mean(1)
    if args.protocol == "monodepth2" and (args.unsupervised or args.mono):        # evaluate_depth.py's line on the median ratios
        med = np.median(ratios)
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)))
    names = ["abs_rel", "sq_rel", "rms", "log_rms", "a1", "a2", "a3"]
    print("Results with scale factor determined by GT/prediction ratio (like the original paper) : ")
    print("{:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}".format(*names))
    print("&{:10.3f}& {:10.3f}& {:10.3f}& {:10.3f}& {:10.3f}& {:10.3f}& {:10.3f}".format(*mean_errors))
    if args.output_dir is not None:
        os.makedirs(args.output_dir, exist_ok=True)
        np.save(os.path.join(args.output_dir, "predictions.npy"), predictions)
    return mean_errors


if __name__ == "__main__":
    main()
