"""Odometry evaluation of the pose networks (eval_pose.py): absolute trajectory error and rotation error on KITTI
odometry sequences, by the two protocols pose networks are compared by.

  sfmlearner   SfMLearner's test_pose.py, which the reference's kitti_eval/pose_evaluation_utils.py was written for: snippets of L
               frames around a target, models.PoseExpNet on (target, references), the L poses re-based on the first frame, scaled to the
               ground truth by least squares; ATE and RE per snippet, mean and std over the snippets.
  monodepth2   monodepth2's evaluate_pose.py: networks.PoseCNN(2) / networks.PoseResnet on consecutive pairs, trajectories of up to 5
               points chained from the pair transforms, scaled by least squares; ATE per window, mean and std over the windows.

This module holds the HOST statement of both -- snippets and ground truth (snippet_indices, compensated_poses: the reference's
read_scene_data / generator, pinned bit for bit by tests/golden/pose_eval.npz), the metrics in numpy fp64 (sfm_metric, mono2_metric) and
the frame arithmetic (host_frame) -- which is what --host-chain runs and what every test measures the device against; and the DEVICE
chain (DevicePoseEvaluator): every frame decoded, uploaded and resized ONCE into a ring of uint8 frames (dn_imresize_u8), snippets
assembled by dn_snippet_gather into one channel-concatenated operand, N snippets through one eval-mode forward, the metric by
dn_pose_eval_sfm / dn_pose_eval_mono2; only [N][2] / [P] doubles come back.

Two stated deviations from the originals:
  * M_k = pose_vec2mat(P_k) and T_i = transformation_from_parameters(...) are formed in fp64 FROM the network's fp32 numbers; the
    originals form them in fp32 (torch) and continue in fp64.  More accurate, and the same on both chains.
  * monodepth2 resizes its frames with Pillow's antialiasing filter; both chains here use scipy.misc.imresize's arithmetic (byte-scale,
    Pillow bilinear: kitti_eval.imresize_bilinear on the host, dn_imresize_u8 on the device), like the sfmlearner protocol.
"""
import ctypes
import os

import numpy as np

from . import kitti_eval as KE

PROTOCOLS = ("sfmlearner", "monodepth2")
POSE_MODELS = ("poseexp", "posecnn", "resnet18")
DEFAULT_PROTOCOL = {"poseexp": "sfmlearner", "posecnn": "monodepth2", "resnet18": "monodepth2"}
ROTATION_MODES = {"euler": 0, "quat": 1}
TRACK_LENGTH = 5                  # evaluate_pose.py: five-frame trajectories, i.e. four pair transforms
MAX_READERS = 16


# ------------------------------------------------------------------------------------------------ snippets and ground truth
def snippet_indices(n_frames, seq_length):
    """pose_evaluation_utils.py:42-56 with step 1 -> int64 [n_frames - 2 demi, seq_length]: rows tgt + (-demi .. demi)."""
    demi = (seq_length - 1) // 2
    shift = np.array([i for i in range(-demi, demi + 1)]).reshape(1, -1)
    tgt = np.arange(demi, n_frames - demi).reshape(-1, 1)
    return shift + tgt


def compensated_poses(poses, indices):
    """pose_evaluation_utils.py:20-23 for one snippet: the L poses [L, 3, 4] fp64 with the first pose's translation subtracted and
    the first pose's rotation undone from the left."""
    p = np.stack([poses[i] for i in indices])
    first = p[0]
    p[:, :, -1] -= first[:, -1]
    return np.linalg.inv(first[:, :3]) @ p


def _list_images(folder, exts):
    return [os.path.join(folder, n) for n in sorted(os.listdir(folder)) if n.rsplit(".", 1)[-1] in exts and os.path.isfile(os.path.join(folder, n))]


def read_sequence(dataset_dir, name, dataset_format="odometry", img_exts=None):
    """-> (image files, poses fp64 [n, 3, 4]).  'odometry': DIR/sequences/<name>/image_2/*.png and DIR/poses/<name>.txt (the reference's
    read_scene_data); 'folders': DIR/<name>/*.jpg and DIR/<name>/poses.txt (what prepare_train_data.py --with-pose writes)."""
    if dataset_format == "odometry":
        files = _list_images(os.path.join(dataset_dir, "sequences", name, "image_2"), img_exts or ("png",))
        pose_file = os.path.join(dataset_dir, "poses", "{}.txt".format(name))
    elif dataset_format == "folders":
        files = _list_images(os.path.join(dataset_dir, name), img_exts or ("jpg",))
        pose_file = os.path.join(dataset_dir, name, "poses.txt")
    else:
        raise ValueError("dataset format '{}' (odometry or folders)".format(dataset_format))
    poses = np.genfromtxt(pose_file).astype(np.float64).reshape(-1, 3, 4)
    if len(poses) != len(files):
        raise ValueError("{}: {} poses for {} frames".format(pose_file, len(poses), len(files)))
    return files, poses


def read_frame(path):
    """One frame as the file holds it, uint8 [H, W, 3]."""
    from PIL import Image
    from .inference import check_frame
    with Image.open(path) as im:
        return check_frame(np.asarray(im), path)


def normalization(protocol):
    """sfmlearner: ((x / 255) - 0.5) / 0.5; monodepth2: x / 255 (ResnetEncoder normalises inside, PoseCNN takes [0, 1])."""
    return ([0.5, 0.5, 0.5], [0.5, 0.5, 0.5]) if protocol == "sfmlearner" else ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def host_frame(frame, size, mean, std):
    """uint8 [H, W, 3] -> normalised fp32 [3, h, w]: scipy.misc.imresize of the float frame unless it has the size already (size None:
    never), then ((x / 255) - mean) / std in fp32, the operation order of dn_snippet_gather."""
    if size is not None and tuple(frame.shape[:2]) != tuple(size):
        frame = KE.imresize_bilinear(frame.astype(np.float32), size)
    x = np.transpose(frame, (2, 0, 1)).astype(np.float32)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    return ((x / np.float32(255)) - m) / s


def sfm_operand_order(indices):
    """Frame indices of a snippet in PoseExpNet's concat order: the target first, then the references in temporal order."""
    idx = [int(i) for i in indices]
    mid = len(idx) // 2
    return [idx[mid]] + idx[:mid] + idx[mid + 1:]


# ------------------------------------------------------------------------------------------------ the metrics, numpy fp64
def pose_vec2mat64(vec, rotation_mode="euler"):
    """inverse_warp.pose_vec2mat (oracle/geometry.py) of fp32 vectors [..., 6] = (tx, ty, tz, rx, ry, rz), evaluated in fp64 -> [..., 3, 4]."""
    v = np.asarray(vec, dtype=np.float32).astype(np.float64)
    lead = v.shape[:-1]
    v = v.reshape(-1, 6)
    x, y, z = v[:, 3], v[:, 4], v[:, 5]
    zero, one = np.zeros_like(x), np.ones_like(x)
    if rotation_mode == "euler":
        cz, sz, cy, sy, cx, sx = np.cos(z), np.sin(z), np.cos(y), np.sin(y), np.cos(x), np.sin(x)
        zm = np.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], 1).reshape(-1, 3, 3)
        ym = np.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], 1).reshape(-1, 3, 3)
        xm = np.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], 1).reshape(-1, 3, 3)
        rot = xm @ ym @ zm
    elif rotation_mode == "quat":
        q = np.stack([one, x, y, z], 1)
        q = q / np.sqrt(np.sum(q * q, axis=1, keepdims=True))
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        w2, x2, y2, z2 = w * w, x * x, y * y, z * z
        wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
        rot = np.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                        2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], 1).reshape(-1, 3, 3)
    else:
        raise ValueError("rotation mode '{}' (euler or quat)".format(rotation_mode))
    return np.concatenate([rot, v[:, :3, None]], 2).reshape(lead + (3, 4))


def sfm_final_poses(pose, rotation_mode="euler"):
    """The network's [L-1, 6] fp32 poses of the reference frames relative to the target -> the L poses [L, 3, 4] fp64 relative to the
    first frame: a zero row for the target at L // 2, M_k inverted, everything re-based on M_0."""
    pose = np.asarray(pose, dtype=np.float32)
    L = pose.shape[0] + 1
    P = np.concatenate([pose[:L // 2], np.zeros((1, 6), np.float32), pose[L // 2:]])
    M = pose_vec2mat64(P, rotation_mode)
    R = np.linalg.inv(M[:, :, :3])
    t = -R @ M[:, :, 3:]
    return np.concatenate([M[0, :, :3] @ R, M[0, :, :3] @ t + M[0, :, 3:]], axis=2)


def sfm_errors(gt, pred):
    """compute_pose_error of SfMLearner's test_pose.py on [L, 3, 4] fp64 poses -> (ATE, RE)."""
    L = gt.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sum(gt[:, :, -1] * pred[:, :, -1]) / np.sum(pred[:, :, -1] ** 2)
        ate = np.linalg.norm((gt[:, :, -1] - scale * pred[:, :, -1]).reshape(-1))
    re = 0.0
    for g, p in zip(gt, pred):
        D = g[:, :3] @ np.linalg.inv(p[:, :3])
        s = np.linalg.norm([D[0, 1] - D[1, 0], D[1, 2] - D[2, 1], D[0, 2] - D[2, 0]])
        re += np.arctan2(s, np.trace(D) - 1)
    return ate / L, re / L


def sfm_metric(pose, gt, rotation_mode="euler"):
    """pose fp32 [N, L-1, 6], gt fp64 [N, L, 3, 4] -> fp64 [N, 2] {ATE, RE}."""
    return np.array([sfm_errors(np.asarray(g, np.float64), sfm_final_poses(p, rotation_mode)) for p, g in zip(pose, gt)], dtype=np.float64).reshape(-1, 2)


def transformation64(pose):
    """layers.transformation_from_parameters(axisangle, translation, invert=False) of fp32 [P, 6] = (axisangle, translation), evaluated in
    fp64 -> [P, 4, 4] = T R: Rodrigues' rotation of axisangle / (|axisangle| + 1e-7), the translation in the last column."""
    v = np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(-1, 6)
    angle = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    axis = v[:, :3] / (angle + 1e-7)[:, None]
    ca, sa = np.cos(angle), np.sin(angle)
    C = 1 - ca
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    xs, ys, zs, xC, yC, zC = x * sa, y * sa, z * sa, x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    T = np.zeros((v.shape[0], 4, 4))
    T[:, 0, 0], T[:, 0, 1], T[:, 0, 2] = x * xC + ca, xyC - zs, zxC + ys
    T[:, 1, 0], T[:, 1, 1], T[:, 1, 2] = xyC + zs, y * yC + ca, yzC - xs
    T[:, 2, 0], T[:, 2, 1], T[:, 2, 2] = zxC - ys, yzC + xs, z * zC + ca
    T[:, :3, 3] = v[:, 3:]
    T[:, 3, 3] = 1
    return T


def to44(poses):
    """[n, 3, 4] -> [n, 4, 4] with the row (0, 0, 0, 1)."""
    G = np.zeros((len(poses), 4, 4))
    G[:, :3] = poses
    G[:, 3, 3] = 1
    return G


def gt_local_transforms(poses):
    """evaluate_pose.py: Q_i = inv(inv(G_i) G_{i+1}) of the 4 x 4 completions of the poses file's rows -> fp64 [n - 1, 4, 4]."""
    G = to44(np.asarray(poses, dtype=np.float64))
    return np.array([np.linalg.inv(np.dot(np.linalg.inv(G[i]), G[i + 1])) for i in range(len(G) - 1)]).reshape(-1, 4, 4)


def dump_xyz(transforms):
    xyzs, cam_to_world = [], np.eye(4)
    xyzs.append(cam_to_world[:3, 3])
    for T in transforms:
        cam_to_world = np.dot(cam_to_world, T)
        xyzs.append(cam_to_world[:3, 3])
    return np.array(xyzs)


def compute_ate(gtruth_xyz, pred_xyz):
    offset = gtruth_xyz[0] - pred_xyz[0]
    pred_xyz = pred_xyz + offset[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sum(gtruth_xyz * pred_xyz) / np.sum(pred_xyz ** 2)
    return np.sqrt(np.sum((pred_xyz * scale - gtruth_xyz) ** 2)) / gtruth_xyz.shape[0]


def mono2_metric(pose, Q, track=TRACK_LENGTH):
    """pose fp32 [P, 6], Q fp64 [P, 4, 4] -> fp64 [P]: the ATE of window i over the transforms i .. min(i + track - 1, P) - 1."""
    T = transformation64(pose)
    P = len(T)
    return np.array([compute_ate(dump_xyz(Q[i:i + track - 1]), dump_xyz(T[i:i + track - 1])) for i in range(P)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ printed results
def format_sfm(errors):
    """errors [N, 2] -> the lines of test_pose.py's table."""
    mean, std = errors.mean(0), errors.std(0)
    return ["Results", "\t {:>10}, {:>10}".format("ATE", "RE"), "mean \t {:10.4f}, {:10.4f}".format(*mean), "std \t {:10.4f}, {:10.4f}".format(*std)]


def format_mono2(ates):
    return ["   Trajectory error: {:0.3f}, std: {:0.3f}".format(np.mean(ates), np.std(ates))]


# ------------------------------------------------------------------------------------------------ the networks
def load_pose_net(pose_model, path, device):
    """-> (network in eval mode on `device`, sequence length)."""
    import torch
    from . import models, networks
    if pose_model == "poseexp":
        weights = torch.load(path, map_location=device)
        seq_length = int(weights["state_dict"]["conv1.0.weight"].size(1) / 3)
        net = models.PoseExpNet(nb_ref_imgs=seq_length - 1, output_exp=False).to(device)
        net.load_state_dict(weights["state_dict"], strict=False)
    elif pose_model == "posecnn":
        state = torch.load(path, map_location=device)
        net, seq_length = networks.PoseCNN(2).to(device), 2
        net.load_state_dict(state.get("state_dict", state))
    elif pose_model == "resnet18":
        net, seq_length = networks.PoseResnet(18).to(device), 2
        net.load_monodepth2(path)
    else:
        raise ValueError("pose model '{}'".format(pose_model))
    net.eval()
    return net, seq_length


def forward_poses(net, dense):
    """One eval-mode forward of N channel-concatenated snippets / pairs [N, 3K, H, W] -> the dense fp32 [N, K-1, 6] on the device.
    PoseExpNet's conv1 takes the 3K channels as ONE operand (run_net(net, dense)), so K - 1 may exceed what forward(target, refs) accepts."""
    import torch
    from .models import PoseExpNet
    from .models._common import run_net
    with torch.no_grad():
        if isinstance(net, PoseExpNet):
            pose = run_net(net, dense)[-1]
        else:
            pose = net(dense)[0]._dn_pose_base
    return pose.reshape(dense.shape[0], -1, 6)


# ------------------------------------------------------------------------------------------------ the two chains
class HostPoseEvaluator(object):
    """--host-chain: the original's loop -- every snippet / pair reads and resizes its own frames, one batch-1 forward, numpy metric."""

    def __init__(self, net, protocol, device, size, rotation_mode="euler"):
        self.net, self.protocol, self.device, self.size, self.rotation_mode = net, protocol, device, size, rotation_mode
        self.mean, self.std = normalization(protocol)

    def _forward(self, files, order):
        import torch
        x = np.concatenate([host_frame(read_frame(files[i]), self.size, self.mean, self.std) for i in order])[None]
        return forward_poses(self.net, torch.from_numpy(np.ascontiguousarray(x)).to(self.device)).cpu().numpy()[0]

    def evaluate(self, files, poses, seq_length):
        """-> (errors: [N, 2] or [P], raw fp32 network outputs [N, L-1, 6] or [P, 6])."""
        if self.protocol == "sfmlearner":
            idx = snippet_indices(len(files), seq_length)
            raw = np.stack([self._forward(files, sfm_operand_order(row)) for row in idx]).astype(np.float32)
            gt = np.stack([compensated_poses(poses, row) for row in idx])
            return sfm_metric(raw, gt, self.rotation_mode), raw
        raw = np.stack([self._forward(files, (i, i + 1)) for i in range(len(files) - 1)]).astype(np.float32).reshape(-1, 6)
        return mono2_metric(raw, gt_local_transforms(poses)), raw


class _Frames(object):
    def __init__(self, files):
        self.files = files

    def __getitem__(self, j):
        return read_frame(self.files[j])


class DevicePoseEvaluator(object):
    """The device chain.  A ring of `capacity` >= batch + K - 1 resized uint8 frames (slot = frame index mod capacity) is filled once
    per frame; per batch: dn_snippet_gather, one forward, (sfmlearner) dn_pose_eval_sfm, and one copy of the results back."""

    def __init__(self, net, protocol, device, size, batch, rotation_mode="euler", readers=4, keep_raw=True):
        import torch
        from .inference import ImageOps
        if batch < 1:
            raise ValueError("batch must be >= 1")
        self.net, self.protocol, self.device, self.size, self.batch = net, protocol, torch.device(device), size, int(batch)
        self.rot = ROTATION_MODES[rotation_mode]
        self.readers = max(1, min(MAX_READERS, int(readers)))
        self.keep_raw = keep_raw
        mean, std = normalization(protocol)
        self.mean_h, self.std_h = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        self.ops = ImageOps(self.device)
        self.ring = None

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _fill_ring(self, frames, first):
        """Resize frames first .. first + len - 1 into their slots: one dn_imresize_u8 per run of slots that does not wrap."""
        import torch
        from . import _lib
        h, w = self.size
        R = self.ring.shape[0]
        done = 0
        while done < len(frames):
            slot = (first + done) % R
            run = frames[done:done + min(len(frames) - done, R - slot)]
            B, _, _, flat, hw, off, idx, taps = self.ops.pack(run, (h, w))
            d_flat, d_hw, d_off, d_idx = (self.ops._upload(n, a) for n, a in (("frames", flat), ("hw", hw), ("off", off), ("tab_idx", idx)))
            minmax = self.ops._buf("minmax", B * 64 * 2, torch.int32)
            _lib.call("dn_imresize_u8", d_flat.data_ptr(), d_hw.data_ptr(), d_off.data_ptr(), B, h, w, self.ops.pool.data_ptr(), d_idx.data_ptr(),
                      taps, minmax.data_ptr(), self.ring[slot].data_ptr(), None, None, None, self._stream())
            done += B

    def evaluate(self, files, poses, seq_length):
        """-> (errors: fp64 [N, 2] or [P], raw fp32 network outputs or None)."""
        import torch
        from . import _lib
        from .evaluation import prefetched
        n = len(files)
        sfm = self.protocol == "sfmlearner"
        if sfm:
            table = np.array([sfm_operand_order(row) for row in snippet_indices(n, seq_length)], dtype=np.int32).reshape(-1, seq_length)
            gt = np.stack([compensated_poses(poses, row) for row in snippet_indices(n, seq_length)]) if len(table) else np.zeros((0, seq_length, 3, 4))
        else:
            table = np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int32)
        count, K = table.shape
        if count == 0:
            return (np.zeros((0, 2)) if sfm else np.zeros((0,))), np.zeros((0, K - 1, 6) if sfm else (0, 6), np.float32)
        frames = prefetched(_Frames(files), n, self.readers, 2 * self.batch + self.readers)
        first = next(frames)
        if self.size is None:
            self.size = tuple(first.shape[:2])
        h, w = self.size
        R = self.batch + K - 1
        if self.ring is None or tuple(self.ring.shape) != (R, h, w, 3):
            self.ring = torch.empty((R, h, w, 3), dtype=torch.uint8, device=self.device)
        pending, loaded = [first], 0
        errors = np.zeros((count, 2) if sfm else (count,), dtype=np.float64)
        raw = np.zeros((count, K - 1, 6), dtype=np.float32) if self.keep_raw else None
        pose_all = None if sfm else torch.empty((count, 6), dtype=torch.float32, device=self.device)
        for s0 in range(0, count, self.batch):
            rows = table[s0:s0 + self.batch]
            nb = len(rows)
            need = int(rows.max()) + 1                      # frames 0 .. need - 1 must have been uploaded
            while loaded + len(pending) < need:
                pending.append(next(frames))
            self._fill_ring(pending, loaded)
            loaded, pending = loaded + len(pending), []
            d_idx = torch.from_numpy(np.ascontiguousarray(rows)).to(self.device)
            d_gt = torch.from_numpy(np.ascontiguousarray(gt[s0:s0 + nb])).to(self.device) if sfm else None
            dense = torch.empty((nb, 3 * K, h, w), dtype=torch.float32, device=self.device)
            st = self._stream()
            _lib.call("dn_snippet_gather", self.ring.data_ptr(), R, d_idx.data_ptr(), nb, K, h, w, self.mean_h, self.std_h, dense.data_ptr(), st)
            pose = forward_poses(self.net, dense).contiguous()
            if sfm:
                out = torch.empty((nb, 2), dtype=torch.float64, device=self.device)
                _lib.call("dn_pose_eval_sfm", pose.data_ptr(), self.rot, d_gt.data_ptr(), nb, K, out.data_ptr(), self._stream())
                errors[s0:s0 + nb] = out.cpu().numpy()
                if raw is not None:
                    raw[s0:s0 + nb] = pose.cpu().numpy()
            else:
                pose_all[s0:s0 + nb] = pose.view(nb, 6)
        if not sfm:
            d_Q = torch.from_numpy(np.ascontiguousarray(gt_local_transforms(poses))).to(self.device)
            out = torch.empty((count,), dtype=torch.float64, device=self.device)
            _lib.call("dn_pose_eval_mono2", pose_all.data_ptr(), d_Q.data_ptr(), count, TRACK_LENGTH, out.data_ptr(), self._stream())
            errors = out.cpu().numpy()
            raw = pose_all.cpu().numpy() if self.keep_raw else None
        return errors, raw


def predictions(protocol, raw, rotation_mode="euler"):
    """What predictions.npy holds: sfmlearner: the final poses [N, L, 3, 4]; monodepth2: the per-pair 4 x 4 transforms [P, 4, 4]."""
    if protocol == "sfmlearner":
        return np.stack([sfm_final_poses(p, rotation_mode) for p in raw]) if len(raw) else np.zeros((0, raw.shape[1] + 1, 3, 4))
    return transformation64(raw)
