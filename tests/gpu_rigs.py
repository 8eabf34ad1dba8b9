"""What the GPU tests of K13, K14 and K15 build on the device for a scene of geometry_scenes.py / voxelize_scenes.py: the passes,
their targets, materials and meshes, and how a scene's draws are recorded; and what the K5 edge tests build for a frame of
shade_maps.py (ShadeRig).  pbrhip is imported where it is used."""
import ctypes as C

ALL = 0xFFFFFFFF


class GeometryRig:
    """G-buffer, post-process (for the velocity targets), geometry pass, materials (the scene's, or PBR_Materials handed in) and one
    single-part PBR_Mesh per draw of a scene."""

    def __init__(self, L, scene, mats=None):
        import pbrhip
        self.L, self.scene = L, scene
        W, H = scene["W"], scene["H"]
        self.gb = pbrhip.PBR_GBuffer()
        L.PBR_MakeGBuffer(C.byref(self.gb), W, H, pbrhip.Format_RGBA16F)
        self.pp = L.PBR_MakePostProcess(C.byref(self.gb), W, H, pbrhip.Format_RGBA8UN)
        self.gp = L.PBR_MakeGeometryPass(C.byref(self.gb), self.pp, W, H)
        assert self.gp
        self.mats = mats or [pbrhip.make_material(m) for m in scene["materials"]]
        self.meshes = []
        for ps in scene["passes"]:
            for d in ps["draws"]:
                v, ix = scene["meshes"][d["mesh"]]
                mesh = pbrhip.make_mesh(v, ix, [(d["first_index"], d["index_count"])])
                L.PBR_MeshSetPartMaterial(mesh, 0, self.mats[d["material"]])
                self.meshes.append(mesh)
        self.bufs = []

    def globals_of(self, d):
        import pbrhip
        g = pbrhip.PBR_Globals()
        for k in range(16):
            g.clip_space_from_world[k] = float(d["m"][k])
            g.old_clip_space_from_world[k] = float(d["m_old"][k])
        return g

    def write_globals(self, d):
        glob = self.globals_of(d)                                             # kept alive across the copy
        C.memmove(self.L.PBR_GeometryGlobalsBuffer(self.gp).contents.data, C.addressof(glob), C.sizeof(glob))

    def record(self, g, frame_idx=0, write_globals=True):
        """One PBR_RecordGeometryPass per pass of the scene when it has one draw; else the raw call sequence (draws of one pass share
        a render-pass instance, each with its own set, buffers and pushed jitter)."""
        import pbrhip
        L, k = self.L, 0
        for ps in self.scene["passes"]:
            draws = ps["draws"]
            d0 = draws[0]
            if write_globals:
                self.write_globals(d0)
            if ps["clear"]:
                L.GPU_OpClearDepthStencil(g, self.gb.depth, ALL)
            L.GPU_OpPrepareRenderPass(g, L.PBR_GeometryRenderPass(self.gp, frame_idx))
            params = [L.GPU_OpPrepareDrawParams(g, L.PBR_GeometryPipeline(self.gp, frame_idx), L.PBR_GeometryDescriptorSet(self.gp, self.mats[d["material"]]))
                      for d in draws]
            L.GPU_OpBeginRenderPass(g)
            for p, d in zip(params, draws):
                mesh = self.meshes[k]
                k += 1
                L.GPU_OpBindVertexBuffer(g, L.PBR_MeshVertexBuffer(mesh))
                L.GPU_OpBindIndexBuffer(g, L.PBR_MeshIndexBuffer(mesh))
                push = (C.c_float * 4)(*d["jitter"], *d["jitter_prev"])
                L.GPU_OpPushGraphicsConstants(g, L.PBR_GeometryLayout(self.gp), push, 16)
                L.GPU_OpBindDrawParams(g, p)
                L.GPU_OpDrawIndexed(g, d["index_count"], 1, d["first_index"], d["vertex_offset"], 0)
            L.GPU_OpEndRenderPass(g)

    def read(self, frame_idx=0):
        import pbrhip
        gb = self.gb
        return dict(base=pbrhip.read_mip(gb.base_color, 0), nrm=pbrhip.read_mip(gb.normal, 0), orm=pbrhip.read_mip(gb.orm, 0),
                    emi=pbrhip.read_mip(gb.emissive, 0), vel=pbrhip.read_mip(self.L.PBR_PostVelocity(self.pp, frame_idx), 0),
                    depth=pbrhip.read_mip(gb.depth, 0)[..., 0].copy())

    def clear_colour(self, g):
        for t in (self.gb.base_color, self.gb.normal, self.gb.orm, self.gb.emissive, self.L.PBR_PostVelocity(self.pp, 0)):
            self.L.GPU_OpClearColorF(g, t, ALL, 0.0, 0.0, 0.0, 0.0)

    def destroy(self):
        L = self.L
        for m in self.meshes:
            L.PBR_DestroyMesh(m)
        L.PBR_DestroyGeometryPass(self.gp)
        for m in self.mats:
            L.PBR_DestroyMaterial(m)
        L.PBR_DestroyPostProcess(self.pp); L.PBR_DestroyGBuffer(C.byref(self.gb))


def voxelize_globals(scene, **over):
    import pbrhip
    g = pbrhip.PBR_Globals()
    sun, sun_dir, scale = over.get("sun", scene["sun"]), over.get("sun_dir", scene["sun_dir"]), over.get("scale", scene["scale"])
    for k in range(16):
        g.sun_space_from_world[k] = float(sun[k])
    for k in range(4):
        g.sun_direction[k] = float(sun_dir[k])
    g.lightgrid_scale = float(scale)
    return g


class VoxelizeRig:
    """Light grid, a sun depth pass whose map is uploaded, the voxelise pass, materials (the scene's, or PBR_Materials handed in) and
    one PBR_Mesh per mesh of a scene."""

    def __init__(self, L, scene, mats=None):
        import pbrhip
        self.L, self.scene = L, scene
        self.lg = L.PBR_MakeLightgrid(scene["N"])
        self.sp = L.PBR_MakeSunDepthPass(scene["sun_map"].shape[0])
        pbrhip.upload_mip(L.PBR_SunDepthTexture(self.sp), 0, scene["sun_map"])
        self.vp = pbrhip.make_voxelize_pass(self.lg, self.sp)
        self.mats = mats or [pbrhip.make_material(m) for m in scene["materials"]]
        self.meshes = [pbrhip.make_mesh(v, ix, [(0, len(ix))]) for v, ix in scene["meshes"]]
        self.tex = L.PBR_LightgridTexture(self.lg)

    def write_globals(self, g):
        C.memmove(self.L.PBR_VoxelizeGlobalsBuffer(self.vp).contents.data, C.addressof(g), C.sizeof(g))

    def record_pass(self, g, ps):
        """The raw call sequence of render.cpp:1039-1056: the draws of one pass share a render-pass instance, each with its own set."""
        L = self.L
        if ps["clear"]:
            L.PBR_RecordLightgridClear(self.lg, g)
        L.GPU_OpPrepareRenderPass(g, L.PBR_VoxelizeRenderPass(self.vp))
        params = [L.GPU_OpPrepareDrawParams(g, L.PBR_VoxelizePipeline(self.vp), L.PBR_VoxelizeDescriptorSet(self.vp, self.meshes[d["mesh"]], self.mats[d["material"]]))
                  for d in ps["draws"]]
        L.GPU_OpBeginRenderPass(g)
        for p, d in zip(params, ps["draws"]):
            L.GPU_OpBindDrawParams(g, p)
            L.GPU_OpDraw(g, d["vertex_count"], d["instance_count"], d["first_vertex"], 0)
        L.GPU_OpEndRenderPass(g)

    def record(self, g, write_globals=True):
        if write_globals:
            self.write_globals(voxelize_globals(self.scene))
        for ps in self.scene["passes"]:
            self.record_pass(g, ps)

    def read(self):
        import pbrhip
        return pbrhip.read_mip(self.tex, 0)

    def destroy(self):
        L = self.L
        L.PBR_DestroyVoxelizePass(self.vp)
        for m in self.meshes:
            L.PBR_DestroyMesh(m)
        for m in self.mats:
            L.PBR_DestroyMaterial(m)
        L.PBR_DestroySunDepthPass(self.sp); L.PBR_DestroyLightgrid(self.lg)


def gpu_format(fmt):
    import pbrhip
    return {"bc1_rgb": pbrhip.Format_BC1_RGB_UN, "bc1_rgba": pbrhip.Format_BC1_RGBA_UN, "bc3": pbrhip.Format_BC3_RGBA_UN, "bc5": pbrhip.Format_BC5_UN}[fmt]


class ShadeRig:
    """K5 on the device for one shade_maps.ShadeCase, with two ways in.  API: PBR_MakeIBLMaps textures whose every level is uploaded
    (no generator runs), a G-buffer with the asked target format, the lighting pass that fits the case (plain, with the sun map, or
    live) and PBR_RecordLightingPass.  Kernel ABI: the same textures' device pointers, twins built here with pbrk_border_build /
    pbrk_cells_build / pbrk_lut_cells_build into device buffers (any of the cells twins may be left NULL), a filled PbrkShadeArgs
    and pbrk_shade(args, NULL)."""

    def __init__(self, L, case, fmt=None):
        import pbrhip
        self.L, self.case = L, case
        W, H = case.W, case.H
        self.fmt = pbrhip.Format_RGBA32F if fmt is None else fmt
        self.maps = pbrhip.PBR_IBLMaps()
        L.PBR_MakeIBLMaps(C.byref(self.maps), case.irr_size, case.lut_size, case.pre)
        assert self.maps.tex_specular_env_map.contents.mip_level_count == len(case.pre_levels)
        for l, lv in enumerate(case.pre_levels):
            pbrhip.upload_mip(self.maps.tex_specular_env_map, l, lv)
        pbrhip.upload_mip(self.maps.irradiance_map, 0, case.irr)
        pbrhip.upload_mip(self.maps.brdf_lut, 0, case.lut)
        self.gb = pbrhip.PBR_GBuffer()
        L.PBR_MakeGBuffer(C.byref(self.gb), W, H, self.fmt)
        for name, key in (("base_color", "base"), ("normal", "normal"), ("orm", "orm"), ("emissive", "emissive"), ("depth", "depth")):
            pbrhip.upload_mip(getattr(self.gb, name), 0, case.gbd[key])
        self.sun_tex = self.grid_tex = self.prev_tex = None
        if case.sun is not None:
            self.sun_tex = pbrhip.make_texture(pbrhip.Format_D32F_Or_X8D24UN, case.sun.shape[1], case.sun.shape[0], pbrhip.TextureFlag_RenderTarget)
            pbrhip.upload_mip(self.sun_tex, 0, case.sun)
        if case.gi:
            n = case.grid.shape[0]
            self.grid_tex = pbrhip.make_texture(pbrhip.Format_RGBA16F, n, n, pbrhip.TextureFlag_StorageImage, depth=n)
            pbrhip.upload_mip(self.grid_tex, 0, case.grid)
            lv0 = case.prev_levels[0]
            self.prev_tex = pbrhip.make_texture(pbrhip.Format_RGBA16F, lv0.shape[1], lv0.shape[0], pbrhip.TextureFlag_RenderTarget | pbrhip.TextureFlag_HasMipmaps)
            assert self.prev_tex.contents.mip_level_count == len(case.prev_levels)
            for m, lv in enumerate(case.prev_levels):
                pbrhip.upload_mip(self.prev_tex, m, lv)
            self.lp = L.PBR_MakeLightingPassLive(C.byref(self.gb), C.byref(self.maps), W, H, self.sun_tex, self.grid_tex, self.prev_tex)
        elif self.sun_tex:
            self.lp = L.PBR_MakeLightingPassEx(C.byref(self.gb), C.byref(self.maps), W, H, self.sun_tex)
        else:
            self.lp = L.PBR_MakeLightingPass(C.byref(self.gb), C.byref(self.maps), W, H)
        assert self.lp
        self.g = L.GPU_MakeGraph()
        self.bufs = {}

    # ---- API ----
    def upload(self, which, array):
        """New content for 'pre<l>', 'irr' or 'lut' through the API (a texture copy: the twins of that texture must follow)."""
        import pbrhip
        if which.startswith("pre"):
            pbrhip.upload_mip(self.maps.tex_specular_env_map, int(which[3:]), array)
        else:
            pbrhip.upload_mip(self.maps.irradiance_map if which == "irr" else self.maps.brdf_lut, 0, array)

    def clear(self, value=-7.0):
        L = self.L
        L.GPU_OpClearColorF(self.g, self.gb.lighting_result, 0, value, value, value, value)
        L.GPU_GraphSubmit(self.g); L.GPU_GraphWait(self.g)

    def read(self):
        import pbrhip
        return pbrhip.read_mip(self.gb.lighting_result, 0).copy()

    def draw_api(self, flags):
        L = self.L
        L.GPUX_SetShadeFlags(L.PBR_LightingPipeline(self.lp), flags)
        L.PBR_RecordLightingPass(self.lp, self.g, C.byref(self.case.glob), 0, 0)
        L.GPU_GraphSubmit(self.g); L.GPU_GraphWait(self.g)
        return self.read()

    # ---- kernel ABI ----
    def _buffer(self, key, nbytes):
        import pbrhip
        if key not in self.bufs:
            self.bufs[key] = self.L.GPU_MakeBuffer(int(nbytes), pbrhip.BufferFlag_GPU, None)
            assert self.bufs[key]
        return self.L.GPUX_BufferDevicePtr(self.bufs[key])

    def build_twins(self):
        """Aprons of both cubes, cells of every prefiltered level (cells_first == 0: for cubes up to 512), level-0 cells of the
        irradiance cube and the LUT's cells, from the textures as they are now.  -> dict of device pointers."""
        L, case = self.L, self.case
        tw = {}
        for key, tex, W, levels in (("pre", self.maps.tex_specular_env_map, case.pre, len(case.pre_levels)), ("irr", self.maps.irradiance_map, case.irr_size, 1)):
            assert W <= 512
            bord = self._buffer(key + "_bordered", L.pbrk_bordered_pyramid_texels(W, levels) * 16)
            assert L.pbrk_border_build(L.GPUX_TextureDevicePtr(tex, 0), bord, W, levels, None) == 0
            sizes = [max(W >> l, 1) for l in range(levels)]
            cells = self._buffer(key + "_cells", sum(L.pbrk_cells_bytes(n) for n in sizes))
            off = 0
            for l, n in enumerate(sizes):
                assert L.pbrk_cells_build(bord + L.pbrk_bordered_level_offset(W, l) * 16, n, cells + off, None) == 0
                off += L.pbrk_cells_bytes(n)
            tw[key + "_bordered"], tw[key + "_cells"] = bord, cells
        S = case.lut_size
        tw["lut_cells"] = self._buffer("lut_cells", (S + 1) * (S + 1) * 16)
        assert L.pbrk_lut_cells_build(L.GPUX_TextureDevicePtr(self.maps.brdf_lut, 0), S, tw["lut_cells"], None) == 0
        L.GPU_WaitUntilIdle()
        return tw

    def args(self, flags, twins, region=None, without=()):
        """PbrkShadeArgs for this frame; `region` = (x0, x1, y0, y1), `without`: names among pre_cells / irr_cells / lut_cells left NULL."""
        import pbrhip
        L, case = self.L, self.case
        a = pbrhip.PbrkShadeArgs()
        a.width, a.height = case.W, case.H
        a.x0, a.x1, a.y0, a.y1 = region if region is not None else (0, case.W, 0, case.H)
        for name in ("base_color", "normal", "orm", "emissive", "depth"):
            setattr(a, name, L.GPUX_TextureDevicePtr(getattr(self.gb, name), 0))
        a.prefiltered_bordered, a.prefiltered_size, a.prefiltered_levels = twins["pre_bordered"], case.pre, len(case.pre_levels)
        a.prefiltered_cells = None if "pre_cells" in without else twins["pre_cells"]
        a.prefiltered_cells_first = 0
        a.irradiance_bordered, a.irradiance_size = twins["irr_bordered"], case.irr_size
        a.irradiance_cells = None if "irr_cells" in without else twins["irr_cells"]
        a.lut, a.lut_size = L.GPUX_TextureDevicePtr(self.maps.brdf_lut, 0), case.lut_size
        a.lut_cells = None if "lut_cells" in without else twins["lut_cells"]
        if self.sun_tex:
            a.sun_depth, a.sun_depth_w, a.sun_depth_h = L.GPUX_TextureDevicePtr(self.sun_tex, 0), case.sun.shape[1], case.sun.shape[0]
        if case.gi:
            a.lightgrid, a.lightgrid_size = L.GPUX_TextureDevicePtr(self.grid_tex, 0), case.grid.shape[0]
            a.prev_frame_levels = len(case.prev_levels)
            a.prev_frame_w, a.prev_frame_h = case.prev_levels[0].shape[1], case.prev_levels[0].shape[0]
            for l in range(a.prev_frame_levels):
                a.prev_frame[l] = L.GPUX_TextureDevicePtr(self.prev_tex, l)
        a.out = L.GPUX_TextureDevicePtr(self.gb.lighting_result, 0)
        a.out_format = pbrhip.PBRK_FMT_RGBA16F if self.fmt == pbrhip.Format_RGBA16F else pbrhip.PBRK_FMT_RGBA32F
        a.flags = flags
        C.memmove(a.globals, C.addressof(case.glob), 552)
        return a

    def shade_abi(self, a):
        """pbrk_shade on the null stream, then idle.  -> the return code."""
        rc = self.L.pbrk_shade(C.byref(a), None)
        self.L.GPU_WaitUntilIdle()
        return rc

    def destroy(self):
        L = self.L
        L.GPU_WaitUntilIdle()
        L.GPU_DestroyGraph(self.g); L.PBR_DestroyLightingPass(self.lp); L.PBR_DestroyGBuffer(C.byref(self.gb)); L.PBR_DestroyIBLMaps(C.byref(self.maps))
        for t in (self.sun_tex, self.grid_tex, self.prev_tex):
            if t:
                L.GPU_DestroyTexture(t)
        for b in self.bufs.values():
            L.GPU_DestroyBuffer(b)
