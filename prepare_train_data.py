#!/usr/bin/env python3
"""KITTI raw in, training folders out -- the command line of the reference's data/prepare_train_data.py:

    python3 prepare_train_data.py KITTI_RAW --dataset-format kitti --dump-root DUMP --width 416 --height 128 --with-depth --with-pose \\
        --test-scenes test_scenes.txt

writes DUMP/<drive>_<cam>/{<frame>.jpg, <frame>.npy, cam.txt, poses.txt} and DUMP/{train,val}.txt, which train.py DUMP and
tools/make_shards.py DUMP read.  The frame resize and the velodyne depth maps run on the device (dn_resize_u8, dn_velo_depth;
supervised_dispnet_amd/kitti_prep.py).

--batch N          frames per device call (default 32).
--readers N        host threads (default 4, at most 16) that decode PNGs and read clouds ahead of the GPU and write the files behind it.
--host-chain       the same files from PIL and numpy on the host; needs no GPU and loads no library.
--test-scenes FILE drives to hold out (the reference's data/test_scenes.txt, which is not shipped here); without it none is.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main(argv=None):
    from supervised_dispnet_amd import kitti_prep
    args = kitti_prep.build_parser().parse_args(argv)           # --help and usage errors need no library
    if not args.host_chain and args.dataset_format == "kitti":
        import __graft_entry__
        __graft_entry__.build(only_library=True)
    return kitti_prep.main(argv)


if __name__ == "__main__":
    main()
