"""What the GPU tests of K13, K14 and K15 build on the device for a scene of geometry_scenes.py / voxelize_scenes.py: the passes,
their targets, materials and meshes, and how a scene's draws are recorded.  pbrhip is imported where it is used."""
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
