"""prepare_train_data.py of the reference (KITTI raw -> the scene folders train.py and tools/make_shards.py read), with the frame resize
and the velodyne depth maps on the device (csrc/dn_image.hip: dn_resize_u8, csrc/dn_velo.hip: dn_velo_depth).

The host side restates data/kitti_raw_loader.py:8-241 in numpy: the calibration readers, pose_from_oxts_packet and the imu2cam pose
chain, the selection of frames by cumulated speed or by a static-frames list, get_P_rect with the zoom of the scene's first frame,
cam.txt (np.savetxt's default format, as the reference writes it) and poses.txt ('%.6e'), the removal of folders with fewer than 3
frames and the 10 % validation split under np.random.seed(8964).  Deviations, all stated here:
  * scipy.misc.imread / imresize / imsave are gone from SciPy: PIL reads, resizes (imresize of a uint8 frame does not stretch it:
    bytescale returns uint8 input unchanged) and writes, which is what those functions called;
  * directories are walked in sorted order (the reference takes the file system's), and the split walks the scene prefixes in SORTED
    order -- the reference walks a set, whose order depends on the interpreter's hash seed -- so a dump is reproducible;
  * test_scenes.txt is the reference's data and is not shipped: --test-scenes FILE names the user's copy; without it no drive is held out;
  * a --height / --width that --depth-size-ratio does not divide is refused (the reference would index past its depth array);
  * --num-threads is accepted and ignored: --readers threads read and write files, one process drives one GPU.

Device chain, per batch of selected frames: ONE upload (frames, their sizes and table indices, clouds, offsets, matrices), dn_resize_u8 and
dn_velo_depth, ONE download (uint8 frames and fp32 maps).  Reader threads decode PNGs and read .bin files ahead of the GPU; the same
threads encode the JPEGs and np.save the maps.  --host-chain writes the same files with PIL and numpy (kitti_eval.project_velodyne /
scatter_depth_min_duplicates with the loader's bounds, rounded to fp32 once); it needs no GPU and loads no library.
"""
import argparse
import os
import shutil
import sys

import numpy as np

from . import kitti_eval as KE

MAX_READERS = 16
DATES = ["2011_09_26", "2011_09_28", "2011_09_29", "2011_09_30", "2011_10_03"]
CAM_IDS = ["02", "03"]


# ------------------------------------------------------------------------------------------------ kitti_raw_loader.py:8-85
def rotx(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def roty(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rotz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def transform_from_rot_trans(R, t):
    return np.vstack((np.hstack([R.reshape(3, 3), t.reshape(3, 1)]), [0, 0, 0, 1]))


def pose_from_oxts_packet(metadata, scale):
    """SE(3) pose of an OXTS packet (lat, lon, alt, roll, pitch, yaw), :35-57 -- with the reference's own ty (no Mercator log)."""
    lat, lon, alt, roll, pitch, yaw = metadata
    er = 6378137.
    ty = lat * np.pi * er / 180.
    tx = scale * lon * np.pi * er / 180.
    t = np.array([tx, ty, alt]).reshape(-1, 1)
    R = rotz(yaw).dot(roty(pitch).dot(rotx(roll)))
    return transform_from_rot_trans(R, t)


def read_raw_calib_file(path):
    """pykitti's reader (:227-241): every line whose values all parse as floats."""
    data = {}
    with open(path, "r") as f:
        for line in f.readlines():
            key, value = line.split(":", 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


# ------------------------------------------------------------------------------------------------ the loader (:87-241)
class KittiRawLoader(object):
    """collect_scenes(drive) -> the scene dictionaries of one drive (one per camera); frames(scene) -> [(index, frame id)] selected;
    velo2im(scene) -> P_velo2im of the scene's depth maps.  No image is decoded here: the zoom needs only the first frame's size."""

    def __init__(self, dataset_dir, static_frames_file=None, img_height=128, img_width=416, min_speed=2, get_depth=False, get_pose=False,
                 depth_size_ratio=1, test_scenes=()):
        self.from_speed = static_frames_file is None
        if static_frames_file is not None:
            self.collect_static_frames(static_frames_file)
        self.test_scenes = list(test_scenes)
        self.dataset_dir = str(dataset_dir)
        self.img_height, self.img_width = img_height, img_width
        self.min_speed, self.get_depth, self.get_pose, self.depth_size_ratio = min_speed, get_depth, get_pose, depth_size_ratio
        self.scenes = []
        for date in DATES:                                                    # collect_train_folders
            folder = os.path.join(self.dataset_dir, date)
            if not os.path.isdir(folder):
                continue
            for name in sorted(os.listdir(folder)):
                if os.path.isdir(os.path.join(folder, name)) and name[:-5] not in self.test_scenes:
                    self.scenes.append(os.path.join(folder, name))

    def collect_static_frames(self, static_frames_file):
        self.static_frames = {}
        with open(static_frames_file, "r") as f:
            for fr in f.readlines():
                if fr == "\n":
                    continue
                date, drive, frame_id = fr.split(" ")
                self.static_frames.setdefault(drive, []).append("%.10d" % int(frame_id[:-1]))

    def image_file(self, scene, i):
        return os.path.join(scene["dir"], "image_" + scene["cid"], "data", scene["frame_id"][i] + ".png")

    def velo_file(self, scene, i):
        return os.path.join(scene["dir"], "velodyne_points", "data", scene["frame_id"][i] + ".bin")

    def collect_scenes(self, drive):
        from PIL import Image
        calib = os.path.dirname(drive)
        oxts_dir = os.path.join(drive, "oxts", "data")
        oxts = sorted(os.path.join(oxts_dir, n) for n in os.listdir(oxts_dir) if n.endswith(".txt"))
        imu2velo = KE.read_calib_file(os.path.join(calib, "calib_imu_to_velo.txt"))
        velo2cam = KE.read_calib_file(os.path.join(calib, "calib_velo_to_cam.txt"))
        cam2cam = KE.read_calib_file(os.path.join(calib, "calib_cam_to_cam.txt"))
        velo2cam_mat = transform_from_rot_trans(velo2cam["R"], velo2cam["T"])
        imu2velo_mat = transform_from_rot_trans(imu2velo["R"], imu2velo["T"])
        cam_2rect_mat = transform_from_rot_trans(cam2cam["R_rect_00"], np.zeros(3))
        imu2cam = cam_2rect_mat @ velo2cam_mat @ imu2velo_mat
        packets = [np.genfromtxt(f) for f in oxts]
        train_scenes = []
        for c in CAM_IDS:
            scene = {"cid": c, "dir": drive, "speed": [], "frame_id": [], "pose": [], "rel_path": os.path.basename(drive) + "_" + c}
            scale = origin = None
            for n, metadata in enumerate(packets):
                scene["speed"].append(metadata[8:11])
                scene["frame_id"].append("{:010d}".format(n))
                if scale is None:
                    scale = np.cos(metadata[0] * np.pi / 180.)
                pose_matrix = pose_from_oxts_packet(metadata[:6], scale)
                if origin is None:
                    origin = pose_matrix
                odo_pose = imu2cam @ np.linalg.inv(origin) @ pose_matrix @ np.linalg.inv(imu2cam)
                scene["pose"].append(odo_pose[:3])
            first = self.image_file(scene, 0) if packets else None
            if first is None or not os.path.isfile(first):
                return []                                                     # as the reference: the whole drive, not this camera
            with Image.open(first) as im:
                W0, H0 = im.size
            scene["P_rect"] = self.get_P_rect(scene, self.img_width / W0, self.img_height / H0)
            scene["intrinsics"] = scene["P_rect"][:, :3]
            train_scenes.append(scene)
        return train_scenes

    def get_P_rect(self, scene, zoom_x, zoom_y):
        filedata = read_raw_calib_file(os.path.join(os.path.dirname(scene["dir"]), "calib_cam_to_cam.txt"))
        P_rect = np.reshape(filedata["P_rect_" + scene["cid"]], (3, 4))
        P_rect[0] *= zoom_x
        P_rect[1] *= zoom_y
        return P_rect

    def frames(self, scene):
        """get_scene_imgs' selection (:193-206) -> [(index, frame id)]."""
        out = []
        if self.from_speed:
            cum_speed = np.zeros(3)
            for i, speed in enumerate(scene["speed"]):
                cum_speed += speed
                if np.linalg.norm(cum_speed) > self.min_speed:
                    out.append((i, scene["frame_id"][i]))
                    cum_speed *= 0
        else:
            drive = os.path.basename(scene["dir"])
            for i, frame_id in enumerate(scene["frame_id"]):
                if (drive not in self.static_frames) or (frame_id not in self.static_frames[drive]):
                    out.append((i, frame_id))
        return out

    def velo_calibration(self, scene):
        """(P_rect / ratio [3, 4], R_rect_00 [9], velo2cam [3, 4]) of generate_depth_map (:250-261)."""
        calib = os.path.dirname(scene["dir"])
        cam2cam = read_raw_calib_file(os.path.join(calib, "calib_cam_to_cam.txt"))
        velo2cam = read_raw_calib_file(os.path.join(calib, "calib_velo_to_cam.txt"))
        rt = np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis]))
        P_rect = np.copy(scene["P_rect"])
        P_rect[0] /= self.depth_size_ratio
        P_rect[1] /= self.depth_size_ratio
        return P_rect, cam2cam["R_rect_00"], rt

    def velo2im(self, scene):
        """P_velo2im (:263): the reference's two np.dot calls."""
        P_rect, r_rect, rt = self.velo_calibration(scene)
        R_cam2rect = np.eye(4)
        R_cam2rect[:3, :3] = r_rect.reshape(3, 3)
        return np.dot(np.dot(P_rect, R_cam2rect), np.vstack((rt, np.array([0, 0, 0, 1.0]))))

    def depth_shape(self):
        """((rows, columns) of a depth map, (lim_h, lim_w) of the in-image test): // against / (:283-288)."""
        r = self.depth_size_ratio
        return (self.img_height // r, self.img_width // r), (self.img_height / r, self.img_width / r)

    def host_depth_map(self, scene, velo):
        """generate_depth_map (:243-300) of one raw cloud fp32 [n, 4] on the host -> fp32 [h, w]."""
        P_rect, r_rect, rt = self.velo_calibration(scene)
        shape, lim = self.depth_shape()
        velo = np.array(velo, dtype=np.float32).reshape(-1, 4)
        velo[:, 3] = 1
        pts = KE.project_velodyne(velo, P_rect, r_rect, rt, lim)
        return KE.scatter_depth_min_duplicates(pts, shape).astype(np.float32)


def read_cloud(path):
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def read_frame(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)


def host_resize(frame, h, w):
    """scipy.misc.imresize(uint8 frame, (h, w)): PIL's bilinear resize, no stretch."""
    from PIL import Image
    return np.asarray(Image.fromarray(frame).resize((int(w), int(h)), resample=Image.BILINEAR))


# ------------------------------------------------------------------------------------------------ the device side
def _put(parts, arr):
    """Append arr's bytes at a 16-byte boundary -> (byte offset, byte count)."""
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    pos = sum(p.size for p in parts)
    parts.append(a)
    pad = -a.size % 16
    if pad:
        parts.append(np.zeros(pad, np.uint8))
    return pos, a.size


def device_batch(ops, frames, size, clouds=None, matrices=None, depth_size=None, lims=None):
    """One batch of the device chain: one upload, dn_resize_u8 [+ dn_velo_depth], one download.
    frames: [H_b x W_b x 3 uint8] or None; size (h, w); clouds: [fp32 [n_b, 4]] or None with matrices fp64 [B, 3, 4], depth_size
    (rows, columns) and lims (lim_h, lim_w).  -> (uint8 [B, h, w, 3] or None, fp32 [B, dh, dw] or None) on the host."""
    import torch
    from . import _lib
    parts, sec = [], {}
    B = len(frames) if frames is not None else len(clouds)
    if frames is not None:
        _, h, w, flat, hw, off, idx, taps = ops.pack(frames, size)
        for name, a in (("frames", flat), ("hw", hw), ("off", off), ("idx", idx)):
            sec[name] = _put(parts, a)
    if clouds is not None:
        clouds = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 4) for c in clouds]
        pt_off = np.zeros(B + 1, dtype=np.int64)
        pt_off[1:] = np.cumsum([len(c) for c in clouds])
        total = int(pt_off[-1])
        dh, dw = int(depth_size[0]), int(depth_size[1])
        for name, a in (("points", np.concatenate(clouds) if total else np.zeros((1, 4), np.float32)), ("pt_off", pt_off),
                        ("M", np.asarray(matrices, dtype=np.float64).reshape(B, 12))):
            sec[name] = _put(parts, a)
    host = np.concatenate(parts)
    dev = ops.workspace("prep_in", host.size)
    dev.copy_(torch.from_numpy(host))                                         # the one upload
    base = dev.data_ptr()
    n_u8 = -(-(B * h * w * 3) // 16) * 16 if frames is not None else 0
    n_f32 = B * dh * dw * 4 if clouds is not None else 0
    out = ops.workspace("prep_out", n_u8 + n_f32)
    if frames is not None:
        ops.resize_packed(B, h, w, base + sec["frames"][0], base + sec["hw"][0], base + sec["off"][0], base + sec["idx"][0], taps,
                          out.data_ptr())
    if clouds is not None:
        need = _lib.load().dn_velo_depth_workspace_bytes(B, dh, dw, total)
        if need == 0:
            raise _lib.DispnetHipError("dn_velo_depth_workspace_bytes refuses B = %d, %d x %d, %d points" % (B, dh, dw, total))
        ws = ops.workspace("velo_ws", need)
        _lib.call("dn_velo_depth", base + sec["points"][0], base + sec["pt_off"][0], total, base + sec["M"][0], B, dh, dw, float(lims[0]),
                  float(lims[1]), ws.data_ptr(), need, out.data_ptr() + n_u8, ops.stream())
    back = out.cpu().numpy()                                                  # the one download
    u8 = back[:B * h * w * 3].reshape(B, h, w, 3) if frames is not None else None
    depth = back[n_u8:n_u8 + n_f32].view(np.float32).reshape(B, dh, dw) if clouds is not None else None
    return u8, depth


# ------------------------------------------------------------------------------------------------ the command line
def build_parser():
    p = argparse.ArgumentParser(description="KITTI raw -> the scene folders train.py reads (the reference's data/prepare_train_data.py)")
    p.add_argument("dataset_dir", metavar="DIR", help="path to original dataset")
    p.add_argument("--dataset-format", type=str, default="kitti", choices=["kitti", "cityscapes"])
    p.add_argument("--static-frames", default=None,
                   help="list of imgs to discard for being static, if not set will discard them based on speed "
                        "(careful, on KITTI some frames have incorrect speed)")
    p.add_argument("--with-depth", action="store_true",
                   help="If available (e.g. with KITTI), will store depth ground truth along with images, for validation")
    p.add_argument("--with-pose", action="store_true",
                   help="If available (e.g. with KITTI), will store pose ground truth along with images, for validation")
    p.add_argument("--no-train-gt", action="store_true", help="If selected, will delete ground truth depth to save space")
    p.add_argument("--dump-root", type=str, default="dump", help="Where to dump the data")
    p.add_argument("--height", type=int, default=128, help="image height")
    p.add_argument("--width", type=int, default=416, help="image width")
    p.add_argument("--depth-size-ratio", type=int, default=1, help="will divide depth size by that ratio")
    p.add_argument("--num-threads", type=int, default=4, help="accepted for the reference's command line; --readers sets the host threads")
    # extensions (not in the reference)
    p.add_argument("--batch", default=32, type=int, metavar="N", help="frames per device call")
    p.add_argument("--readers", default=4, type=int, metavar="N", help="host threads that read and write files (at most 16)")
    p.add_argument("--host-chain", action="store_true", help="resize and depth maps in PIL / numpy on the host: the same files, no GPU")
    p.add_argument("--test-scenes", default=None, metavar="FILE", help="drives to hold out, one per line (the reference's test_scenes.txt)")
    return p


def _read_item(loader, item, with_depth):
    scene, i, _ = item
    frame = read_frame(loader.image_file(scene, i))
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError("{}: a frame of shape {} and type {} -- RGB uint8 frames only".format(loader.image_file(scene, i), frame.shape,
                                                                                            frame.dtype))
    return frame, (read_cloud(loader.velo_file(scene, i)) if with_depth else None)


def _write_item(dump_root, item, img, depth):
    from PIL import Image
    scene, _, frame_id = item
    folder = os.path.join(dump_root, scene["rel_path"])
    Image.fromarray(img).save(os.path.join(folder, "{}.jpg".format(frame_id)))        # scipy.misc.imsave of a uint8 array
    if depth is not None:
        np.save(os.path.join(folder, "{}.npy".format(frame_id)), depth)


def _host_item(loader, dump_root, item, with_depth):
    frame, cloud = _read_item(loader, item, with_depth)
    depth = loader.host_depth_map(item[0], cloud) if with_depth else None
    _write_item(dump_root, item, host_resize(frame, loader.img_height, loader.img_width), depth)


def dump_frames(args, loader, items):
    """Resize, depth maps and files for every selected frame: [(scene, index, frame id)]."""
    import collections
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=args.readers) as pool:
        if args.host_chain:
            for f in [pool.submit(_host_item, loader, args.dump_root, it, args.with_depth) for it in items]:
                f.result()
            return
        import torch
        from .inference import ImageOps
        ops = ImageOps(torch.device("cuda"))
        shape, lims = loader.depth_shape()
        matrices = {}
        ahead = 2 * args.batch + args.readers
        reads, writes, nxt = collections.deque(), collections.deque(), 0
        for j0 in range(0, len(items), args.batch):
            chunk = items[j0:j0 + args.batch]
            while nxt < len(items) and nxt < j0 + ahead:
                reads.append(pool.submit(_read_item, loader, items[nxt], args.with_depth))
                nxt += 1
            got = [reads.popleft().result() for _ in chunk]
            if args.with_depth:
                for scene, _, _ in chunk:
                    if scene["rel_path"] not in matrices:
                        matrices[scene["rel_path"]] = loader.velo2im(scene)
                u8, depth = device_batch(ops, [g[0] for g in got], (args.height, args.width), [g[1] for g in got],
                                         np.stack([matrices[s["rel_path"]] for s, _, _ in chunk]), shape, lims)
            else:
                u8, depth = device_batch(ops, [g[0] for g in got], (args.height, args.width))
            for k, it in enumerate(chunk):
                writes.append(pool.submit(_write_item, args.dump_root, it, u8[k], depth[k] if depth is not None else None))
            while len(writes) > ahead:
                writes.popleft().result()
        for f in writes:
            f.result()


def main(argv=None):
    """-> {"scenes": [folders kept], "frames": frames written}."""
    args = build_parser().parse_args(argv)
    if args.dataset_format == "cityscapes":
        raise SystemExit("prepare_train_data.py: --dataset-format cityscapes is not implemented (only the KITTI raw loader is built)")
    r = args.depth_size_ratio
    if r < 1 or args.height % r or args.width % r:
        raise SystemExit("prepare_train_data.py: --height {} and --width {} must be multiples of --depth-size-ratio {} (the reference indexes "
                         "past its depth array otherwise)".format(args.height, args.width, r))
    if args.batch < 1:
        raise SystemExit("prepare_train_data.py: --batch must be >= 1")
    if not 1 <= args.readers <= MAX_READERS:
        clamped = max(1, min(MAX_READERS, args.readers))
        print("prepare_train_data.py: warning: --readers {} is outside 1..{}; using {}".format(args.readers, MAX_READERS, clamped),
              file=sys.stderr)
        args.readers = clamped
    if args.test_scenes is not None:
        with open(args.test_scenes, "r") as f:
            test_scenes = [t.strip() for t in f if t.strip()]
    else:
        test_scenes = []
        print("prepare_train_data.py: warning: no --test-scenes FILE, so no drive is held out of the training folders", file=sys.stderr)
    if not args.host_chain:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prepare_train_data.py drives the MI355X HIP path; no GPU is visible (--host-chain runs on the host)")
    loader = KittiRawLoader(args.dataset_dir, static_frames_file=args.static_frames, img_height=args.height, img_width=args.width,
                            get_depth=args.with_depth, get_pose=args.with_pose, depth_size_ratio=r, test_scenes=test_scenes)
    os.makedirs(args.dump_root, exist_ok=True)
    print("Retrieving frames")
    scenes, items = [], []
    for drive in loader.scenes:
        for scene in loader.collect_scenes(drive):
            folder = os.path.join(args.dump_root, scene["rel_path"])
            os.makedirs(folder, exist_ok=True)
            np.savetxt(os.path.join(folder, "cam.txt"), scene["intrinsics"])
            picked = loader.frames(scene)
            if args.with_pose and picked:
                poses = [scene["pose"][i].tolist() for i, _ in picked]
                np.savetxt(os.path.join(folder, "poses.txt"), np.array(poses).reshape(-1, 12), fmt="%.6e")
            scenes.append((scene, len(picked)))
            items += [(scene, i, frame_id) for i, frame_id in picked]
    dump_frames(args, loader, items)
    kept = []
    for scene, _ in scenes:
        folder = os.path.join(args.dump_root, scene["rel_path"])
        if len([n for n in os.listdir(folder) if n.endswith(".jpg")]) < 3:
            shutil.rmtree(folder)
        else:
            kept.append(scene["rel_path"])
    print("Generating train val lists")
    np.random.seed(8964)
    subdirs = sorted(n for n in os.listdir(args.dump_root) if os.path.isdir(os.path.join(args.dump_root, n)))
    with open(os.path.join(args.dump_root, "train.txt"), "w") as tf, open(os.path.join(args.dump_root, "val.txt"), "w") as vf:
        for pr in sorted(set(n[:-2] for n in subdirs)):                       # two cameras of a drive fall into the same set
            corresponding = [n for n in subdirs if n.startswith(pr)]
            if np.random.random() < 0.1:
                for s in corresponding:
                    vf.write("{}\n".format(s))
            else:
                for s in corresponding:
                    tf.write("{}\n".format(s))
                    if args.with_depth and args.no_train_gt:
                        folder = os.path.join(args.dump_root, s)
                        for n in os.listdir(folder):
                            if n.endswith(".npy"):
                                os.remove(os.path.join(folder, n))
    return {"scenes": kept, "frames": len(items)}
