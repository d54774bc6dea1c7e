#!/usr/bin/env python3
"""Render a scene file on the MI355X without the reference's frontend: the reference's own scene.json (+ _data.bin), a
glTF / GLB, or one of the built-in procedural workloads, through the whole chain — ingestion (libptamd scene_io), path
tracing (GMoN optional), fused post-process + tonemap — to an 8-bit PNG.

    python tools/render_scene.py tests/golden/scene_fixture/mini.json out.png --size 640 360 --spp 64
    python tools/render_scene.py model.glb out.png --camera-pos 0 1.5 6 --camera-target 0 1 0 --env sky
    python tools/render_scene.py builtin:c5 out.png --size 960 540 --spp 32 --bounces 12
    python tools/render_scene.py builtin:c1 preview.png --size 640 640 --spp 1 --denoise --despeckle
    python tools/render_scene.py builtin:c5 out.png --size 960 540 --spp 32 --auto-exposure
    python tools/render_scene.py builtin:c5 out.png --size 960 540 --spp 32 --auto-exposure --bloom 0.1
    python tools/render_scene.py builtin:c3 corner.png --size 1920 1080 --spp 4096 --region 1200,600,1500,800
    python tools/render_scene.py builtin:c3 out.png --size 960 540 --spp 32 --matte instance      (writes out.instance.png beside out.png)
    python tools/render_scene.py builtin:c3 out.png --size 960 540 --spp 32 --select 497,498,530 --outline-width 3
    python tools/render_scene.py builtin:c5 cutout.png --size 960 540 --spp 64 --film transparent     (an RGBA PNG with straight alpha)
    python tools/render_scene.py builtin:c5 studio.png --size 960 540 --spp 64 --film 0.18,0.18,0.18  (the objects over a flat colour)
    python tools/render_scene.py builtin:c1 clay.png --size 640 640 --spp 64 --ao 2      (writes clay_ao.png beside clay.png: dark corners, white walls)
    python tools/render_scene.py builtin:c3 ids.png --size 960 540 --spp 32 --view matte --matte instance   (the picture itself shows the ids)
    python tools/render_scene.py builtin:c3 heat.png --size 960 540 --spp 256 --adaptive 0.05 --view samples --ramp heat
    python tools/render_scene.py builtin:c5 probe.png --size 1024 512 --spp 64 --projection equirect     (a light probe of the scene)
    python tools/render_scene.py builtin:c5 dome.png --size 1024 1024 --spp 64 --projection fisheye --fisheye-fov 3.14159
    python tools/render_scene.py model.glb evening.png --env daylight --sun-elevation 8 --sun-azimuth 200 --turbidity 3 --auto-exposure
    python tools/render_scene.py plan.gltf plan.png --projection ortho --ortho-height 12     (a glTF orthographic camera is used as it is)
"""
import argparse, os, struct, sys, time, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from platinum_amd import Renderer, abi, scene_io, scenes
import png


def write_png_rgba8(path, img):
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def matte_false_colour(slots, n):
    """(H, W, 3) float image of one matte layer: every slot's id hashed to a colour (the background, abi.MATTE_NONE, black), weighted by
    count / n; samples that found no slot (more than abi.MATTE_SLOTS ids in a pixel) add nothing.  slots (H, W, MATTE_SLOTS), n (H, W)."""
    ids = slots["id"].astype(np.uint64)
    h = (ids * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF          # Knuth's multiplicative hash: neighbouring ids get unrelated colours
    rgb = np.stack([(h >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.float32) / 255.0 * 0.85 + 0.15
    rgb[slots["id"] == abi.MATTE_NONE] = 0.0
    w = slots["count"].astype(np.float32) / np.maximum(n, 1).astype(np.float32)[..., None]
    return (rgb * w[..., None]).sum(axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene"); ap.add_argument("output")
    ap.add_argument("--size", type=int, nargs=2, default=(960, 540))
    ap.add_argument("--spp", type=int, default=64); ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--gmon", type=int, default=0, help="GMoN bucket count (0 = plain mean)")
    ap.add_argument("--camera-pos", type=float, nargs=3); ap.add_argument("--camera-target", type=float, nargs=3, default=(0, 0, 0))
    ap.add_argument("--focal", type=float, default=28.0)
    ap.add_argument("--env", default="none", help="'sky' = procedural sky, 'daylight' = a physical sun and sky generated on the device (see "
                                                  "--sun-elevation), or the path of an .exr / Radiance .hdr environment map")
    ap.add_argument("--sun-elevation", type=float, default=30.0, metavar="DEG", help="with --env daylight: the sun's height over the horizon, -90 .. 90")
    ap.add_argument("--sun-azimuth", type=float, default=0.0, metavar="DEG", help="with --env daylight: the sun's azimuth (0 = towards -x, 90 = towards -z)")
    ap.add_argument("--sun-size", type=float, default=0.27, metavar="DEG", help="with --env daylight: the sun's angular radius")
    ap.add_argument("--turbidity", type=float, default=1.0, metavar="D", help="with --env daylight: dust density relative to a clear day, 0 .. 10")
    ap.add_argument("--sky-size", default="1024x512", metavar="WxH", help="with --env daylight: the size of the generated environment map")
    ap.add_argument("--exposure", type=float, default=0.0)
    ap.add_argument("--auto-exposure", type=float, nargs="?", const=-2.4739313, default=None, metavar="TARGET_LOG2",
                    help="meter the image's luminance histogram and bring its mean to 2^TARGET_LOG2 (default log2 0.18) ahead of the post-process; "
                         "--exposure acts on top as compensation")
    ap.add_argument("--bloom", type=float, nargs="?", const=0.05, default=None, metavar="INTENSITY",
                    help="scatter this fraction of the light (default 0.05) with a wide glare pyramid, after --auto-exposure and ahead of the post-process")
    ap.add_argument("--denoise", action="store_true", help="keep first-hit AOVs and write the image through the a-trous denoiser")
    ap.add_argument("--despeckle", type=float, nargs="?", const=2.0, default=None, metavar="T",
                    help="with --denoise: clamp a pixel brighter than T x its brightest 3x3 neighbour ahead of the filter (fireflies; default T = 2)")
    ap.add_argument("--adaptive", type=float, default=None, metavar="THRESHOLD",
                    help="tile-adaptive sampling: an 8x8 tile stops once every pixel's relative error is <= THRESHOLD (--spp is the maximum)")
    ap.add_argument("--region", default=None, metavar="X0,Y0,X1,Y1",
                    help="render region: sample only the pixels [X0, X1) x [Y0, Y1) (top-left origin); the rest of the image stays empty (alpha 0)")
    ap.add_argument("--matte", choices=("instance", "material"), action="append", default=[],
                    help="keep ID mattes and write a false-colour image of this layer beside the picture (OUTPUT.instance.png / OUTPUT.material.png): "
                         "what every pixel's camera rays hit first, each id a colour, weighted by its share of the pixel's samples; may be given twice")
    ap.add_argument("--select", default=None, metavar="ID[,ID...]",
                    help="keep ID mattes and draw the selection overlay, an outline around these ids, onto the picture after the post-process")
    ap.add_argument("--select-layer", choices=("instance", "material"), default="instance", help="what the ids of --select are")
    ap.add_argument("--outline-width", type=float, default=2.0, metavar="W", help="width of the outline in pixels, 1 .. 16")
    ap.add_argument("--film", default=None, metavar="transparent|R,G,B",
                    help="keep the transparent film and show the objects without the environment behind them: 'transparent' writes straight alpha "
                         "into the PNG, R,G,B (scene-linear, >= 0) puts that flat colour behind them; the environment still lights the scene")
    ap.add_argument("--ao", type=float, nargs="?", const=1.0, default=None, metavar="DISTANCE",
                    help="keep the ambient-occlusion pass (one occlusion ray of at most DISTANCE world units, default 1, 'inf' allowed, from every "
                         "camera ray's first hit) and write it in grey beside the picture: OUTPUT_ao.png, white = open")
    ap.add_argument("--view", choices=abi.VIEW_NAMES, default="beauty",
                    help="what the picture shows (the render target's pass view, drawn on the device): the beauty, or the albedo, normals, depth, "
                         "film alpha, ID mattes (the layer of --matte, default instance), sample counts or noise estimate; what the view needs is kept")
    ap.add_argument("--ramp", choices=("grey", "heat"), default="grey", help="with --view depth / samples / noise: grey, or blue-cyan-green-yellow-red")
    ap.add_argument("--projection", choices=abi.PROJ_NAMES, default=None,
                    help="the camera's projection: perspective (the default, unless the scene's camera is a glTF orthographic one), ortho, equirect "
                         "(a panorama: 2:1 with the default --pano-fov is a light probe of the scene) or fisheye (equidistant)")
    ap.add_argument("--ortho-height", type=float, default=None, metavar="H", help="with --projection ortho: height of the view volume in world units")
    ap.add_argument("--pano-fov", type=float, nargs=2, default=None, metavar=("X", "Y"),
                    help="with --projection equirect: radians covered horizontally (0, 2 pi] and vertically (0, pi]")
    ap.add_argument("--fisheye-fov", type=float, default=None, metavar="A",
                    help="with --projection fisheye: full angle in radians reached at the edge of the image's shorter side, (0, 2 pi]")
    a = ap.parse_args()
    for flag, value, kind in (("--ortho-height", a.ortho_height, "ortho"), ("--pano-fov", a.pano_fov, "equirect"), ("--fisheye-fov", a.fisheye_fov, "fisheye")):
        if value is not None and a.projection != kind:
            ap.error("%s needs --projection %s" % (flag, kind))
    view = abi.VIEW_NAMES.index(a.view)
    backdrop = None
    if a.film is not None and a.film != "transparent":
        try:
            backdrop = tuple(float(v) for v in a.film.split(","))
        except ValueError:
            backdrop = ()
        if len(backdrop) != 3 or not all(0.0 <= v < float("inf") for v in backdrop):
            ap.error("--film takes 'transparent' or R,G,B with finite components >= 0")
    select = None
    if a.select is not None:
        try:
            select = [int(v, 0) for v in a.select.split(",")]
        except ValueError:
            select = []
        if not select or min(select) < 0 or max(select) > 0xFFFFFFFF or not 1.0 <= a.outline_width <= 16.0:
            ap.error("--select takes ID[,ID...] (0xFFFFFFFF = the background) and --outline-width a width from 1 to 16")
    if a.ao is not None and not a.ao > 0.0:
        ap.error("--ao takes a distance > 0 (inf allowed)")
    if a.despeckle is not None and not a.denoise:
        ap.error("--despeckle is a stage of the denoiser: it needs --denoise")
    region = None
    if a.region is not None:
        try:
            region = tuple(int(v) for v in a.region.split(","))
        except ValueError:
            region = ()
        if len(region) != 4 or min(region) < 0 or region[0] >= region[2] or region[1] >= region[3] or region[2] > a.size[0] or region[3] > a.size[1]:
            ap.error("--region takes X0,Y0,X1,Y1 with 0 <= X0 < X1 <= width and 0 <= Y0 < Y1 <= height")
        if a.gmon > 1:
            ap.error("--region does not combine with --gmon")
    t0 = time.time()
    if a.scene.startswith("builtin:"):
        factory, *_ = scenes.CONFIGS[a.scene.split(":", 1)[1]]
        sc = factory()
    else:
        sc = scene_io.SceneFile.load(a.scene) if a.scene.endswith(".json") else scene_io.SceneFile.empty().import_gltf(
            a.scene, scene_io.GLTF_SKIP_EMPTY_NODES | scene_io.GLTF_ORTHOGRAPHIC_CAMERAS)
        if a.env == "sky":
            sc.set_environment(scenes.sky_environment(1024, 512))
        elif a.env not in ("none", "daylight"):
            sc.load_environment(a.env)
        if a.camera_pos is not None or not sc.cameras():
            sc.add_camera(a.camera_pos or (0.0, 1.5, 6.0), a.camera_target, a.focal)
        c = sc.counts()
        print(f"scene: {c.instances} instances, {c.triangles} triangles, {c.textures} textures, {c.materials} materials, cameras {sc.cameras()}")
    r = Renderer(device=0)
    if a.env == "daylight":   # (a built-in scene takes it too: it replaces the scene's own environment)
        try:
            sky_w, sky_h = (int(v) for v in a.sky_size.lower().split("x"))
            sky, ss = r.generateSky(width=sky_w, height=sky_h, stats=True, sun_elevation=np.radians(a.sun_elevation), sun_azimuth=np.radians(a.sun_azimuth),
                                    sun_angular_radius=np.radians(a.sun_size), dust_density=a.turbidity)
        except (ValueError, abi.PtamdError) as e:
            ap.error("--env daylight: %s" % e)
        sc.set_environment(sky)
        print(f"daylight: {sky_w} x {sky_h} in {ss.kernel_ms:.2f} ms on the device; the sun covers {ss.sun_texels} texels "
              f"({ss.sun_solid_angle:.3g} sr, radius {np.degrees(ss.sun_radius_used):.3g} deg)")
    # the projection: the scene camera's own (a glTF orthographic camera), with the command line over it
    proj = sc.camera_projection() if isinstance(sc, scene_io.SceneFile) else r.projection()
    if a.projection is not None:
        proj.kind = abi.PROJ_NAMES.index(a.projection)
    if a.ortho_height is not None:
        proj.ortho_height = a.ortho_height
    if a.pano_fov is not None:
        proj.fov_x, proj.fov_y = a.pano_fov
    if a.fisheye_fov is not None:
        proj.fisheye_fov = a.fisheye_fov
    try:
        r.setProjection(proj)
    except abi.PtamdError as e:
        ap.error(str(e))
    if a.denoise:
        r.setDenoiseOptions(enabled=1, apply_to_target=1)
    if a.despeckle is not None:
        r.setDespeckleOptions(enabled=1, threshold=a.despeckle)
    if a.auto_exposure is not None:
        r.setExposureOptions(enabled=1, target_log2=a.auto_exposure)
    if a.bloom is not None:
        r.setBloomOptions(enabled=1, intensity=a.bloom)
    if a.adaptive is not None:
        if a.gmon > 1:
            ap.error("--adaptive does not combine with --gmon")
        r.setAdaptiveOptions(enabled=1, threshold=a.adaptive)
    if region is not None:
        r.setRenderRegion(*region)
    if a.matte or select or view == abi.VIEW_MATTE:
        r.setMatteOptions(enabled=1)
    if view in (abi.VIEW_ALBEDO, abi.VIEW_NORMAL, abi.VIEW_DEPTH) or (view == abi.VIEW_NOISE and a.adaptive is None):
        r.setDenoiseOptions(enabled=1)       # (keeps the AOVs; the filter runs only with --denoise)
    if select:
        r.setSelectionOptions(enabled=1, layer=abi.MATTE_INSTANCE if a.select_layer == "instance" else abi.MATTE_MATERIAL, width=a.outline_width)
        r.setSelection(select)
    if a.ao is not None:
        r.setAmbientOcclusionOptions(enabled=1, distance=a.ao)
    if a.film is not None:
        r.setFilmOptions(enabled=1, backdrop=abi.BACKDROP_TRANSPARENT if backdrop is None else abi.BACKDROP_COLOR, backdrop_rgb=backdrop or (0.0, 0.0, 0.0))
    elif view == abi.VIEW_ALPHA:
        r.setFilmOptions(enabled=1)
    if view != abi.VIEW_BEAUTY:
        r.setViewOptions(view=view, ramp=abi.RAMP_HEAT if a.ramp == "heat" else abi.RAMP_GREY,
                         layer=abi.MATTE_MATERIAL if a.matte[:1] == ["material"] else abi.MATTE_INSTANCE)
    flags = abi.FLAG_MULTISCATTER_GGX | (abi.FLAG_GMON if a.gmon > 1 else 0)
    r.startRender(sc, tuple(a.size), a.spp, gmonBuckets=max(1, a.gmon), flags=flags, max_bounces=a.bounces, nonfinite_policy=abi.NONFINITE_ZERO)
    t1 = time.time()
    r.render(0); r.wait()
    t2 = time.time()
    po = r.postProcessOptions(); po.exposure = a.exposure
    r.setPostProcessOptions(po)
    img = r.readbackRenderTarget()
    write_png_rgba8(a.output, img)
    if view != abi.VIEW_BEAUTY:
        vs = r.viewStats()
        print(f"view: {abi.VIEW_NAMES[vs.shown]}" + (f", depth {vs.depth_min:.4g} .. {vs.depth_max:.4g} over {vs.depth_pixels} pixels" if vs.shown == abi.VIEW_DEPTH else ""))
    if a.auto_exposure is not None:
        m = r.readbackExposureMeter()   # (no smoothing: the ev a read resolves now is the one the image above got)
        print(f"auto exposure: {m.metered} pixels metered ({m.below} below, {m.above} above, {m.nonfinite} non-finite), mean log2 luminance {m.mean_log2:.3f}, "
              f"applied {m.ev:+.3f} EV (gain {m.gain:.4g})")
    if a.film is not None:
        alpha = r.readbackFilm()[..., 3]
        print(f"film: coverage 1 on {int((alpha == 1).sum())} pixels, 0 on {int((alpha == 0).sum())}, fractional on {int(((alpha > 0) & (alpha < 1)).sum())}; "
              + ("straight alpha written" if backdrop is None else "backdrop %g, %g, %g" % backdrop))
    if a.ao is not None:
        ao = r.readbackAmbientOcclusion()
        path = os.path.splitext(a.output)[0] + "_ao.png"
        g = np.round(np.clip(ao, 0.0, 1.0) * 255.0).astype(np.uint8)     # linear grey: a data pass, not a picture
        write_png_rgba8(path, np.stack([g, g, g, np.full_like(g, 255)], axis=-1))
        s_ao = r.ambientOcclusionStats()
        print(f"ambient occlusion: wrote {path}; distance {a.ao:g}, {s_ao.rays} AO rays, mean {float(ao.mean()):.3f}, {int((ao == 1).sum())} pixels fully open")
    if select:
        cov = r.readbackMatte(r.selectionOptions().layer, select)
        print(f"selection: {len(r.selection())} {a.select_layer} ids cover {int((cov > 0).sum())} pixels ({float(cov.sum()):.1f} in all), outline {a.outline_width:g} px")
    for layer in dict.fromkeys(a.matte):
        slots = r.readbackMatteSlots(abi.MATTE_INSTANCE if layer == "instance" else abi.MATTE_MATERIAL)
        n = r.readbackSampleCounts()
        path = os.path.splitext(a.output)[0] + "." + layer + ".png"
        # (png.write_png shows x / (1 + x) to the power 1 / 2.2: handed the inverse, the colours come out as computed)
        c = np.clip(matte_false_colour(slots, n), 0.0, 0.999) ** 2.2
        png.write_png(path, c / (1.0 - c))
        other = int((n.astype(np.int64) - slots["count"].sum(axis=-1)).sum())
        print(f"matte: wrote {path}; {np.unique(slots['id'][slots['count'] != 0]).size} distinct {layer} ids, "
              f"{other} of {int(n.sum())} samples beyond the {abi.MATTE_SLOTS} slots of their pixel")
    st = r.stats()
    print(f"setup {t1 - t0:.2f} s (BVH {st.bvh_build_ms:.1f} ms), render {t2 - t1:.3f} s = {a.size[0] * a.size[1] * a.spp * a.bounces / (t2 - t1) / 1e6:.0f} Msamples/s, wrote {a.output}")
    if a.adaptive is not None:
        n = r.readbackSampleCounts()
        if region is not None:
            n = n[region[1]:region[3], region[0]:region[2]]
        print(f"adaptive: {st.paths} paths = {st.paths / (n.size * a.spp):.3f} of uniform, per-pixel samples {n.min()}..{n.max()}, mean {n.mean():.1f}")
    if region is not None:
        area = (region[2] - region[0]) * (region[3] - region[1])
        print(f"region: {area} of {a.size[0] * a.size[1]} pixels; {st.paths} paths = {st.paths / (a.size[0] * a.size[1] * a.spp):.4f} of the full frame's {a.size[0] * a.size[1] * a.spp}")


if __name__ == "__main__":
    main()
