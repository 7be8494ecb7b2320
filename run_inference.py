#!/usr/bin/env python3
"""Pictures in, disparity and depth images out -- the command line of the reference's run_inference.py (:19-38), running the network
on the MI355X HIP path and the image arithmetic around it on the device:

    python3 run_inference.py --pretrained CKPT --network disp_vgg_BN --dataset-dir FRAMES --output-disp --output-depth

writes OUT/network/timestamp/{j}_disp.ext (the Garg-crop rectangle of the disparity, 'bone'), {j}_en.ext (its contrast-4 enhancement)
and {namebase}_depth.ext (1 / disparity, max_value 10, 'rainbow').

--batch N      images per forward (default 8); resize, normalise, colouring and contrast run on the device
               (supervised_dispnet_amd/inference.py).
--readers K    host threads (default 4, at most 16) that read files ahead of the GPU.
--host-chain   the reference's per-image chain in numpy / PIL on the host: the same forward, the same files.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main(argv=None, **kw):
    from supervised_dispnet_amd import inference
    args = inference.build_parser().parse_args(argv)            # --help and usage errors need no library
    del args
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    return inference.main(argv, **kw)


if __name__ == "__main__":
    main()
