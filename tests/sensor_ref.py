"""The yardstick of the sensor filters (ht_sensor_*): a numpy restatement of RSCam's depth filters, read against the reference's include/dcam.h:157-226
and written as its own sequential loops -- no code and no decomposition shared with csrc/ht_sensor.hip.  tests/test_sensor_ref.py pins it.

A frame is u16 [h, w], an IR image u8 [h, w], a camera 12 float32 (focal xy, principal xy, depth_scale, pose 7)."""
import numpy as np

IVY, DS4 = 0, 1
DARK = 4096


def out_dims(kind, w, h, max_width=320):
    """(w_out, h_out) after the halving loop `while (dim.x > image_width_max_allowed) DownSampleFst` (dcam.h:205-206, 212-213); ValueError for what ht_sensor_out_dims refuses"""
    if kind not in (IVY, DS4) or not (1 <= w <= 4096 and 1 <= h <= 4096) or max_width < 1:
        raise ValueError("kind, size or max_width")
    k = 0
    while (w >> k) > max_width:
        k += 1
    if kind == DS4 and k:
        raise ValueError("a DS4 frame wider than max_width: the reference reads outside its halved IR image")
    if w % (1 << k) or h % (1 << k):
        raise ValueError("DownSample reads past an image whose size is odd")
    return w >> k, h >> k


def downsample_fst(img):
    """DownSampleFst (misc_image.h:81-94): the first pixel of every 2x2, as the reference's loop writes it"""
    h, w = img.shape
    dw, dh = w // 2, h // 2
    dst = np.zeros((dh, dw), img.dtype)
    for y in range(0, h, 2):
        for x in range(0, w, 2):
            dst[y // 2, x // 2] = img[y, x]
    return dst


def halve_cam(cam):
    """DCamera / 2 (misc_image.h:62): focal and principal halved in float, depth_scale and pose kept"""
    c = np.array(cam, np.float32)
    c[:4] = c[:4] / np.float32(2.0)
    return c


def ivy_fill(depth_scale):
    """(unsigned short)(4.0f / depth_scale) (dcam.h:216) as the x86 build forms it: the float quotient, a truncating conversion to int32 (INT_MIN when it
    does not fit), its low 16 bits"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.float32(4.0) / np.float32(depth_scale)
    v = int(q) if np.isfinite(q) and -2147483648.0 <= float(q) < 2147483648.0 else -2147483648
    return v & 0xFFFF


def filter_ivy(depth, cam, max_width=320):
    """FilterIvy (dcam.h:209-226) by its definition: k halvings, output pixel (x, y) = input pixel (x * 2^k, y * 2^k), the camera halved k times, then 0 -> 4 m"""
    h, w = depth.shape
    wo, ho = out_dims(IVY, w, h, max_width)
    k = (w // wo).bit_length() - 1
    out = np.zeros((ho, wo), np.uint16)
    for y in range(ho):
        for x in range(wo):
            out[y, x] = depth[y << k, x << k]
    c = np.array(cam, np.float32)
    for _ in range(k):
        c = halve_cam(c)
    out[out == 0] = ivy_fill(c[4])
    return out, c


def filter_ivy_loops(depth, cam, max_width=320):
    """FilterIvy as the reference runs it: DownSampleFst while the image is too wide, then the fill"""
    img, c = np.array(depth, np.uint16), np.array(cam, np.float32)
    while img.shape[1] > max_width:
        img, c = downsample_fst(img), halve_cam(c)
    fill = ivy_fill(c[4])
    flat = img.reshape(-1)
    for i in range(flat.size):
        if flat[i] == 0:
            flat[i] = fill
    return img, c


def ds4_pass1(depth, ir):
    """dcam.h:182-188: dark in IR or nearer than 30 counts -> 4096"""
    return [DARK if (d < 30 or l < 8) else d for d, l in zip(np.asarray(depth).reshape(-1).tolist(), np.asarray(ir).reshape(-1).tolist())]


def filter_ds4(depth, ir, background=None, max_width=320):
    """FilterDS4 (dcam.h:174-208): the three loops in the reference's order, the second one rewriting p in place in raster order"""
    h, w = depth.shape
    out_dims(DS4, w, h, max_width)
    p = ds4_pass1(depth, ir)

    def hasneighbor(i, stride):
        return abs(p[i + stride] - p[i]) < 10 or abs(p[i - stride] - p[i]) < 10

    for i in range(w * h):
        x, y = i % w, i // w
        if x < 2 or x >= w - 2 or y < 2 or y >= h - 2:
            continue
        if not hasneighbor(i, 1) or not hasneighbor(i, w) or not hasneighbor(i, 2) or not hasneighbor(i, w * 2):
            p[i] = DARK
    if background is not None:
        bg = np.asarray(background).reshape(-1).tolist()
        for i in range(w * h):
            if p[i] > bg[i]:
                p[i] = DARK
    return np.array(p, np.uint16).reshape(h, w)


def add_background(background, depth, fudge=3):
    """addbackground (dcam.h:157-162): background None is the model before the first call (4096 everywhere); dp[i] - fudge in int, the cast wrapping"""
    d = np.asarray(depth).reshape(-1).tolist()
    bg = [DARK] * len(d) if background is None else np.asarray(background).reshape(-1).tolist()
    for i in range(len(d)):
        bg[i] = min(bg[i], (d[i] - fudge) & 0xFFFF)
    return np.array(bg, np.uint16).reshape(np.asarray(depth).shape)
