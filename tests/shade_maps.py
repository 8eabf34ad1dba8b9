"""Map contents for the K5 edge tests (test_gpu_shade_edges.py, test_shade_maps_cpu.py), computed on the CPU for any face size
n >= 1: cube levels whose value says which face, level, channel and texel it came from, an RG16F LUT with its own gradient in u
and in v, and the wild-byte G-buffer of test_shade_random_bytes_all_decodes.  The maps are pure numpy; ShadeCase adds the frame's other
inputs, the oracle frame for them and the conditioning screen (CPU only: PBR_FillGlobals and the oracle, no GPU call).

A level is  field(direction) * k(face, level, channel) * checker(i, j):  the field is smooth and positive, k is different for
every face, level and channel (a tap from the wrong one is off by several per cent) and the checker is +-2 % over (i + j) & 1, so
that adjacent texels differ by about 4 % (a tap that is off by one texel is off by hundreds of tolerances)."""
import numpy as np

CHECKER = 0.02
CHANNEL = (1.0, 0.88, 1.12)


def level_count(n):
    c = 1
    while n > 1:
        n >>= 1
        c += 1
    return c


def level_sizes(n):
    return [max(n >> l, 1) for l in range(level_count(n))]


def _field(d, variant):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    p = 0.9 * variant
    return 1.6 + 0.7 * np.sin(2.1 * x + 0.3 + p) * np.cos(1.7 * y - p) + 0.4 * np.sin(2.9 * z + 1.0 + 2.0 * p)     # [0.5, 2.7]


def factor(face, level, channel, variant=0):
    return (0.85 + 0.06 * ((face + 2 * variant) % 6)) * (1.2 - 0.04 * ((level + 3 * variant) % 11)) * CHANNEL[(channel + variant) % 3]


def cube_level(n, level=0, variant=0):
    """One cube level, float32 [6][n][n][4] (face, row, column, rgba), alpha 1.  `level` and `variant` only select the content."""
    from pbrhip import synth
    f = _field(synth.face_dirs(n), variant)                                       # [6][n][n]
    j, i = np.mgrid[0:n, 0:n]
    f = f * (1.0 + CHECKER * (1 - 2 * ((i + j) & 1)))
    out = np.ones((6, n, n, 4), np.float32)
    for face in range(6):
        for c in range(3):
            out[face, :, :, c] = f[face] * factor(face, level, c, variant)
    return out


def cube_pyramid(n, variant=0):
    """Every level of a cube of face size n (n, n >> 1, ..., 1): list of [6][n_l][n_l][4] float32."""
    return [cube_level(m, l, variant) for l, m in enumerate(level_sizes(n))]


def pyramid_flat(levels):
    return np.concatenate([lv.ravel() for lv in levels])


def lut(size, variant=0):
    """RG16F LUT, float16 [size][size][2] (row = v, column = u): r rises with u, g falls with v, both inside (0, 1)."""
    c = (np.arange(size) + 0.5) / size
    u, v = np.meshgrid(c, c, indexing="xy")
    r = 0.15 + 0.7 * u + 0.1 * v
    g = 0.6 - 0.45 * v + 0.05 * u
    if variant:
        r, g = 0.9 - 0.6 * u + 0.05 * v, 0.1 + 0.5 * v + 0.1 * u
    return np.stack([r, g], -1).astype(np.float16)


def wild_gbuffer(W, H, seed):
    """Random base, normal, orm and emissive bytes (non-unit normals, every roughness), depth in [0.9980, 0.9999], ~20 % sky."""
    rng = np.random.default_rng(seed)
    gbd = {k: rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for k in ("base", "normal", "orm", "emissive")}
    gbd["emissive"][rng.random((H, W)) > 0.1] = 0
    depth = (0.9980 + 0.0019 * rng.random((H, W))).astype(np.float32)
    depth[rng.random((H, W)) < 0.2] = 1.0
    gbd["depth"] = depth
    return gbd


IBL, SHAFTS, SHADOWS, GI = 1, 2, 4, 8            # PBRK_SHADE_* == pbrhip.Shade_*
CAMERA = (0.3, -0.2, 5.0)                        # off every axis: each component has an ulp that means something
REL, FLOOR = 1e-4, 1e-2                          # the suite's criterion for K5: rel_err(got, want, floor=1e-2) < 1e-4
SCREEN_MOVE, SCREEN_CAP = 1e-5, 0.005
SEED = 0x5EED0E02                                # wild bytes of every frame below: the screen removes 0 to 3 surface pixels (test_shade_maps_cpu.py)
RAGGED = ((1, 1), (63, 3), (65, 5), (130, 9))    # one pixel; under / over one 64-wide workgroup, rows not a multiple of 4; three workgroups wide
RAGGED_GI = ((37, 13), (93, 53))                 # partial 8 x 8 waves and partial 32 x 8 workgroups in x and in y
FAST_FLAGS = (0, SHAFTS, IBL, IBL | SHAFTS)      # k_shade_fast<kIBL, kShafts>
GENERAL_FLAGS = (IBL, 0, SHAFTS, IBL | SHADOWS, SHAFTS | SHADOWS)
GI_FLAGS = (SHAFTS | SHADOWS | GI, IBL | GI)


def rel_map(a, b, floor=FLOOR):
    """Per-pixel max over rgb of |a - b| / max(|b|, floor), float64 [H][W]."""
    a = np.asarray(a, np.float64)[..., :3]; b = np.asarray(b, np.float64)[..., :3]
    return (np.abs(a - b) / np.maximum(np.abs(b), floor)).max(-1)


class ShadeCase:
    """Host side of one K5 frame: G-buffer (wild bytes of `seed`, or synth_gi_scene with gi=True), maps of shade_maps, Globals, and
    with shadows=True a 64^2 rippled sun depth map centred on the surface pixels' depth as the sun sees them."""

    def __init__(self, W, H, pre, irr, lut_size, seed=SEED, gi=False, shadows=False, frame_idx=17):
        import pbrhip
        from pbrhip import synth
        self.W, self.H, self.pre, self.irr_size, self.lut_size, self.gi = W, H, pre, irr, lut_size, gi
        self.pre_levels = cube_pyramid(pre)
        self.irr = cube_level(irr, 0, variant=1)
        self.lut = lut(lut_size)
        self.sun = self.grid = self.prev_levels = None
        self._ref = {}
        if gi:
            self.gbd, self.grid, levels, self.sun = _gi_scene(W, H)
            self.prev_levels = levels[:min(level_count(min(levels[0].shape[0], levels[0].shape[1])), 8)]      # the texture's chain ends with its short side
            self.glob = pbrhip.fill_globals(synth.GI_SCENE_CAMERA, aspect=W / H, frame_idx=3)
            self.glob.lightgrid_scale = 1.0 / synth.GI_SCENE_EXTENT
        else:
            self.gbd = wild_gbuffer(W, H, seed)
            self.glob = pbrhip.fill_globals(CAMERA, aspect=W / H, frame_idx=frame_idx)
        g32 = np.frombuffer(bytes(self.glob), np.float32)
        M = lambda k: g32[16 * k:16 * k + 16].reshape(4, 4).T.astype(np.float64)
        ys, xs = np.mgrid[0:H, 0:W]
        ndc = np.stack([(xs + 0.5) / W * 2 - 1, (ys + 0.5) / H * 2 - 1, self.gbd["depth"].astype(np.float64), np.ones((H, W))], -1)
        pw = ndc @ M(2).T                                                        # world_space_from_clip
        P = pw[..., :3] / pw[..., 3:]
        self.surface = (np.abs(P) <= 99.0).all(-1)                               # lighting_pass.glsl:708, in float64
        self.roughness4 = self.gbd["orm"][..., 1].astype(np.float64) / 255.0 * 4.0
        if shadows and not gi:
            ps = np.concatenate([P[self.surface], np.ones((int(self.surface.sum()), 1))], 1) @ M(6).T      # sun_space_from_world
            z = ps[:, 2] if len(ps) else np.array([0.5])
            self.sun = sun_ripples(64, float(np.median(z)), float(max(np.percentile(z, 75) - np.percentile(z, 25), 1e-3)))

    def set_maps(self, which, variant):
        """Other content for one map: 'pre<l>' (one level of the prefiltered cube), 'irr' or 'lut'.  Returns the new array."""
        self._ref = {}
        if which.startswith("pre"):
            l = int(which[3:])
            self.pre_levels[l] = cube_level(self.pre_levels[l].shape[1], l, variant)
            return self.pre_levels[l]
        if which == "irr":
            self.irr = cube_level(self.irr_size, 0, variant)
            return self.irr
        self.lut = lut(self.lut_size, variant)
        return self.lut

    def oracle(self, flags, region=None, camera=None):
        """The oracle frame, float32 [H][W][4]; `region` = (x0, x1, y0, y1): 0 outside it.  `camera` replaces Globals.camera_pos only."""
        import pbr_oracle as O
        og = O.OrcGlobals.from_buffer_copy(bytes(self.glob))
        if camera is not None:
            og.camera_pos[:] = [float(v) for v in camera]
        of = (O.SHADE_IBL if flags & IBL else 0) | (O.SHADE_SHAFTS if flags & SHAFTS else 0) | (O.SHADE_SHADOWS if flags & SHADOWS else 0) | \
             (O.SHADE_GI if flags & GI else 0)
        g = self.gbd
        return O.shade(og, g["base"], g["normal"], g["orm"], g["emissive"], g["depth"], flags=of, irradiance_cube=self.irr,
                       prefiltered_pyr=pyramid_flat(self.pre_levels), prefiltered_size=self.pre, lut_half=self.lut.view(np.uint16), region=region,
                       sun_depth_map=self.sun if flags & (SHADOWS | GI) else None, lightgrid=self.grid if flags & GI else None,
                       prev_frame_levels=self.prev_levels if flags & GI else None)

    def screen(self, flags, want=None):
        """Conditioning screen: the pixels whose oracle value moves by more than 1e-5 (relative, floor 1e-2) when one non-zero camera
        component moves by one ulp either way are where the shader itself is ill-conditioned (the GGX sun term at low roughness), not
        where a kernel can be told from the oracle.  Returns (keep [H][W] bool, share of the surface pixels removed); sky pixels are
        always kept, and the share is asserted to stay under the 0.5 % cap."""
        want = self.oracle(flags) if want is None else want
        cam = np.array(list(self.glob.camera_pos), np.float32)
        moved = np.zeros((self.H, self.W), bool)
        for k in range(3):
            if cam[k] == 0:
                continue
            for to in (np.float32(np.inf), np.float32(-np.inf)):
                c = cam.copy()
                c[k] = np.nextafter(cam[k], to)
                moved |= rel_map(self.oracle(flags, camera=c), want) > SCREEN_MOVE
        moved &= self.surface
        n = max(int(self.surface.sum()), 1)
        share = float(moved.sum()) / n
        assert share <= SCREEN_CAP, (share, int(moved.sum()), n)
        return ~moved, share


    def reference(self, flags):
        """(oracle frame, keep mask, share of surface pixels the screen removed), computed once per flag set and map content.  The GI
        scene is compared on every pixel (its arithmetic is exact by design): no screen."""
        if flags not in self._ref:
            want = self.oracle(flags)
            keep, share = (np.ones((self.H, self.W), bool), 0.0) if flags & GI else self.screen(flags, want)
            self._ref[flags] = (want, keep, share)
        return self._ref[flags]


_GI = {}


def _gi_scene(W, H):
    from pbrhip import synth
    if (W, H) not in _GI:
        _GI[(W, H)] = synth.synth_gi_scene(W, H)
    return _GI[(W, H)]


def sun_ripples(size, centre, amplitude):
    """A size^2 sun depth map: ripples of `amplitude` around `centre`, a few periods across the map (lit and shadowed pixels both occur)."""
    v, u = np.mgrid[0:size, 0:size] / float(size)
    return (centre + amplitude * np.sin(2 * np.pi * 5 * u) * np.cos(2 * np.pi * 4 * v)).astype(np.float32)
