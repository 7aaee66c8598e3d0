"""Frames as a lens sees them: synth.Scene ray-cast through the radial model of DESIGN.md section 17, in float64.  For every pixel of the
DISTORTED frame the radial map x_d = k(x_u) x_u is inverted by fixed-point iteration (60 steps converge for every lens here), and the
height field is ray-cast along the ideal ray through x_u exactly as Scene.render does for the regular grid.  Independent of
tests/lens_mirror.py (which maps the other way, in float32)."""
import numpy as np

import tracks_yaml
from mvs_amd import synth


def _file_lens(name):
    t = tracks_yaml.load(name)
    return tuple(t["distortion"])


def lenses(W, H):
    """name -> (k, centre in pixels with y from the bottom): the two bundled real lenses (coefficients as the tracks files give them), a
    pincushion, and a barrel with a third coefficient around an off-centre principal point"""
    mid = (W / 2.0, H / 2.0)
    return {
        "koberec": (_file_lens("koberec.yaml"), mid),
        "zatisi": (_file_lens("zatisi.yaml"), mid),
        "pincushion": ((0.08, 0.0, 0.0), mid),
        "offcentre": ((-0.12, 0.05, 0.02), (0.47 * W, 0.55 * H)),
    }


LENS_NAMES = ("koberec", "zatisi", "pincushion", "offcentre")


def ideal_coordinates(W, H, k, center=None, iterations=60):
    """(xn, yn), [H, W] float64: the undistorted normalised coordinates whose image under the lens is the pixel centre (row, col) of the
    distorted frame"""
    k = list(k) + [0.0] * (3 - len(k))
    cx, cy = (W / 2.0, H / 2.0) if center is None else center
    a = H / W
    X = (np.arange(W, dtype=np.float64) + 0.5)[None, :].repeat(H, 0)
    Y = (np.arange(H, dtype=np.float64) + 0.5)[:, None].repeat(W, 1)
    xd = (X - cx) * 2.0 / W
    yd = ((H - cy) - Y) * 2.0 / H
    xu, yu = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = (xu * xu + yu * yu * a * a) / 4.0
        kf = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
        xu, yu = xd / kf, yd / kf
    return xu, yu


def render_rays(scene, cam_center, xn, yn, W, H, fovx=synth.FOVX):
    """Scene.render's ray-cast for arbitrary normalised coordinates (the regular grid gives Scene.render's image)"""
    cx, cy, cz = [float(c) for c in cam_center]
    dx = xn * fovx / 2.0
    dy = yn * fovx / (2.0 * (W / H))
    t = np.full(xn.shape, 3.0 + cz)
    for _ in range(14):
        t = cz - scene.height(cx + t * dx, cy + t * dy)
    return np.clip(np.rint(scene.albedo(cx + t * dx, cy + t * dy)), 0, 255).astype(np.uint8)


def render_through_lens(scene, cam_center, W, H, k, center=None):
    xn, yn = ideal_coordinates(W, H, k, center)
    return render_rays(scene, cam_center, xn, yn, W, H)


def make_views(W, H, V, k, center=None, radius=0.15):
    """synth.make_views with every frame seen through the lens: (main_cam, main_img, side_cams, side_imgs, main_depth_ndc); cameras and
    depth are the pinhole ones"""
    sc = synth.Scene(synth.SEED_SCENE, W / 1920.0)
    main_cam, side_cams = synth.ring_cameras(V, W, H, radius)
    _, depth = sc.render([0, 0, 0], W, H, want_depth=True)
    xn, yn = ideal_coordinates(W, H, k, center)
    main_img = render_rays(sc, [0, 0, 0], xn, yn, W, H)
    sides = []
    for v in range(V):
        a = 2.0 * np.pi * v / max(V, 1)
        sides.append(render_rays(sc, [radius * np.cos(a), radius * np.sin(a), 0.0], xn, yn, W, H))
    return main_cam, main_img, side_cams, sides, depth


def noise(W, H, seed=7):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W), dtype=np.uint8)


def checkerboard(W, H):
    """0 / 255 in squares of 4 x 4 pixels: next to their edges the bicubic kernel overshoots both ways (below 0 and above 255)"""
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((xx >> 2) + (yy >> 2)) & 1) * 255).astype(np.uint8)
