#!/usr/bin/env python3
"""Odometry evaluation of the pose networks: absolute trajectory error (and rotation error) on KITTI odometry sequences,

    python3 eval_pose.py --pretrained-posenet exp_pose_checkpoint.pth.tar --dataset-dir KITTI_ODOMETRY --sequences 09 10
    python3 eval_pose.py --pretrained-posenet mono_640x192/ --pose-model resnet18 --dataset-dir KITTI_ODOMETRY --sequences 09 10 \
        --img-height 192 --img-width 640
    python3 eval_pose.py --pretrained-posenet pose.pth --pose-model posecnn --dataset-dir DUMP --dataset-format folders \
        --sequences 2011_09_26_drive_0001_sync_02

--pose-model poseexp  a .pth.tar with `state_dict` of models.PoseExpNet (sequence length = conv1.0.weight.size(1) / 3), evaluated by
                      SfMLearner's protocol: snippets of L frames, ATE and RE per snippet, the table `ATE, RE` with mean and std.
--pose-model posecnn  a monodepth2 pose.pth of networks.PoseCNN(2);
--pose-model resnet18 a monodepth2 folder (pose_encoder.pth + pose.pth) of networks.PoseResnet(18); both evaluated by monodepth2's
                      protocol: consecutive pairs, trajectories of 5 frames, `Trajectory error: mean, std`.
--dataset-format      odometry: DIR/sequences/<seq>/image_2/*.png and DIR/poses/<seq>.txt; folders: DIR/<scene>/*.jpg and
                      DIR/<scene>/poses.txt, what prepare_train_data.py --with-pose writes (--sequences then names scene folders).
--batch N             snippets / pairs per forward on the device chain: every frame is decoded, uploaded and resized once into a ring of
                      resident frames, snippets are gathered on the device (dn_snippet_gather), N of them take one eval-mode forward,
                      and the metric runs on the device (dn_pose_eval_sfm / dn_pose_eval_mono2); supervised_dispnet_amd/pose_eval.py,
                      DESIGN.md section 21.
--host-chain          the original's loop instead: each snippet reads and resizes its own frames on the host, one forward per snippet,
                      the metric in numpy.  Same networks, same definition; the yardstick of the device chain.
--output-dir DIR      saves predictions.npy: the final poses [N, L, 3, 4] (sfmlearner) or the per-pair 4 x 4 transforms (monodepth2).
--dump-poses FILE     saves the raw fp32 network outputs in snippet / pair order (np.save).
With more than one sequence each gets its own block of output, and the arrays of the sequences are concatenated in the files.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

from supervised_dispnet_amd import pose_eval as PE  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Odometry evaluation (ATE / RE) of the pose networks on KITTI odometry sequences",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter, allow_abbrev=False)
    p.add_argument("--pretrained-posenet", required=True, type=str, help="pose network weights: a .pth.tar (poseexp), a pose.pth (posecnn) "
                   "or a monodepth2 folder (resnet18)")
    p.add_argument("--pose-model", default="poseexp", choices=PE.POSE_MODELS, help="which pose network the weights belong to")
    p.add_argument("--protocol", default=None, choices=PE.PROTOCOLS, help="evaluation protocol; default: sfmlearner for poseexp, monodepth2 "
                   "for posecnn and resnet18")
    p.add_argument("--dataset-dir", default=".", type=str, help="dataset directory")
    p.add_argument("--sequences", default=["09"], type=str, nargs="*", help="sequences (odometry) or scene folders (folders) to test")
    p.add_argument("--dataset-format", default="odometry", choices=("odometry", "folders"), help="layout of --dataset-dir")
    p.add_argument("--img-height", default=128, type=int, help="image height the network takes")
    p.add_argument("--img-width", default=416, type=int, help="image width the network takes")
    p.add_argument("--no-resize", action="store_true", help="no resizing is done")
    p.add_argument("--rotation-mode", default="euler", choices=("euler", "quat"), help="rotation the poseexp outputs encode")
    p.add_argument("--img-exts", default=None, nargs="*", type=str, help="image extensions to list (default: png for odometry, jpg for folders)")
    p.add_argument("--batch", default=32, type=int, metavar="N", help="snippets / pairs per forward on the device chain")
    p.add_argument("--readers", default=4, type=int, metavar="R", help="host threads that decode frames ahead of the GPU (at most 16)")
    p.add_argument("--host-chain", action="store_true", help="the original's per-snippet loop: host resize, one forward per snippet, numpy metric")
    p.add_argument("--output-dir", default=None, type=str, help="saves predictions.npy there")
    p.add_argument("--dump-poses", default=None, type=str, metavar="FILE", help="saves the raw fp32 network outputs in snippet / pair order")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.protocol is None:
        args.protocol = PE.DEFAULT_PROTOCOL[args.pose_model]
    if (args.pose_model == "poseexp") != (args.protocol == "sfmlearner"):
        raise SystemExit("eval_pose.py: --pose-model {} is evaluated by the {} protocol, not by {}".format(
            args.pose_model, PE.DEFAULT_PROTOCOL[args.pose_model], args.protocol))
    if args.batch < 1:
        raise SystemExit("eval_pose.py: --batch must be >= 1")
    if args.pose_model == "resnet18" and not os.path.isdir(args.pretrained_posenet):
        raise SystemExit("eval_pose.py: --pose-model resnet18 takes a monodepth2 FOLDER (pose_encoder.pth and pose.pth), got '{}'".format(
            args.pretrained_posenet))
    if args.pose_model != "resnet18" and not os.path.isfile(args.pretrained_posenet):
        raise SystemExit("eval_pose.py: --pose-model {} takes a weights FILE, got '{}'".format(args.pose_model, args.pretrained_posenet))
    if not args.sequences:
        raise SystemExit("eval_pose.py: --sequences needs at least one name")
    args.readers = max(1, min(PE.MAX_READERS, args.readers))
    return args


def main(argv=None):
    """-> {sequence: errors} (fp64 [N, 2] {ATE, RE} per snippet, or [P] ATE per window)."""
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_pose.py drives the MI355X HIP path; no GPU is visible (there is no CPU fallback)")
    device = torch.device("cuda")
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    net, seq_length = PE.load_pose_net(args.pose_model, args.pretrained_posenet, device)
    size = None if args.no_resize else (args.img_height, args.img_width)
    keep_raw = args.dump_poses is not None or args.output_dir is not None
    if args.host_chain:
        evaluator = PE.HostPoseEvaluator(net, args.protocol, device, size, args.rotation_mode)
    else:
        evaluator = PE.DevicePoseEvaluator(net, args.protocol, device, size, args.batch, args.rotation_mode, args.readers, keep_raw)
    results, raws = {}, []
    for name in args.sequences:
        files, poses = PE.read_sequence(args.dataset_dir, name, args.dataset_format, args.img_exts)
        errors, raw = evaluator.evaluate(files, poses, seq_length)
        results[name] = errors
        raws.append(raw)
        if len(args.sequences) > 1:
            print("sequence {}: {} frames, {} {}".format(name, len(files), len(errors), "snippets" if args.protocol == "sfmlearner" else "windows"))
        else:
            print("{} {} to test".format(len(errors), "snippets" if args.protocol == "sfmlearner" else "windows"))
        for line in (PE.format_sfm(errors) if args.protocol == "sfmlearner" else PE.format_mono2(errors)):
            print(line)
    if keep_raw:
        raw = np.concatenate(raws)
        if args.dump_poses is not None:
            np.save(args.dump_poses, raw)
        if args.output_dir is not None:
            os.makedirs(args.output_dir, exist_ok=True)
            np.save(os.path.join(args.output_dir, "predictions.npy"), PE.predictions(args.protocol, raw, args.rotation_mode))
    return results


if __name__ == "__main__":
    main()
