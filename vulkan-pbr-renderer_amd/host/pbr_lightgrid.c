/*
 * pbr_lightgrid.c -- host side of the voxel light grid: its sweep and the voxelise pass that fills it (N7), the
 * GPU_* call sequence of
 *   render.cpp:678          the 128^3 RGBA16F storage image
 *   render.cpp:816          its "IMG0" storage-image binding in the main pass layout
 *   render.cpp:151-187      the sweep compute pipeline + descriptor set (only IMG0 is read by the shader;
 *                           the reference fills the layout's other slots with dummies it calls "stupid")
 *   render.cpp:1028         frame-0 clear
 *   render.cpp:1061-1072    per frame: advance sweep_direction, push it, GPU_OpDispatch(1, 16, 16)
 *   render.cpp:113-149      the voxelise pipeline (lightgrid_voxelize.glsl, conservative rasterisation, no vertex inputs)
 *   render.cpp:711-714      its N x N render pass without targets
 *   asset_import.cpp:196-204  a part's descriptor set: SSBO0 / SSBO1 = the mesh's buffers, IMG0 = the grid, TEX0 / TEX_EMISSIVE,
 *                           the sun depth map and the samplers
 *   render.cpp:1039-1056    PrepareRenderPass, PrepareDrawParams per part, BeginRenderPass, BindDrawParams + GPU_OpDraw per part
 * The backend rasterises the voxelise pass with K14.
 */
#include "pbr_host.h"
#include "pbr_mesh.h"

#include <stdlib.h>
#include <string.h>

struct PBR_Lightgrid {
    GPU_Texture* lightgrid;
    GPU_PipelineLayout* layout;
    uint32_t img0_binding;
    GPU_ComputePipeline* sweep_pipeline;
    GPU_DescriptorSet* sweep_desc_set;
    uint32_t sweep_direction;            /* render.h:204 (zero-initialised, incremented before use) */
};

PBR_Lightgrid* PBR_MakeLightgrid(uint32_t size) {
    PBR_Lightgrid* lg = (PBR_Lightgrid*)calloc(1, sizeof *lg);
    lg->lightgrid = GPU_MakeTexture(GPU_Format_RGBA16F, size, size, size, GPU_TextureFlag_StorageImage, NULL);   /* render.cpp:678 */
    lg->layout = GPU_InitPipelineLayout();
    lg->img0_binding = GPU_StorageImageBinding(lg->layout, "IMG0", lg->lightgrid->format);                       /* render.cpp:816 */
    GPU_FinalizePipelineLayout(lg->layout);

    /* render.cpp:156-162 */
    static const char path[] = "../src/demo_pbr_renderer/shaders/lightgrid_sweep.glsl";
    GPU_Access cs_accesses[] = { GPU_ReadWrite(lg->img0_binding) };
    GPU_ShaderDesc cs_desc; memset(&cs_desc, 0, sizeof cs_desc);
    cs_desc.accesses = cs_accesses; cs_desc.accesses_count = 1;
    cs_desc.glsl_debug_filepath.data = path; cs_desc.glsl_debug_filepath.length = sizeof path - 1;
    GPU_GLSLErrorArray errors = {0};
    cs_desc.spirv = GPU_SPIRVFromGLSL(NULL, GPU_ShaderStage_Compute, lg->layout, &cs_desc, &errors);
    lg->sweep_pipeline = GPU_MakeComputePipeline(lg->layout, &cs_desc);

    /* render.cpp:164-165, 186 */
    lg->sweep_desc_set = GPU_InitDescriptorSet(NULL, lg->layout);
    GPU_SetStorageImageBinding(lg->sweep_desc_set, lg->img0_binding, lg->lightgrid, 0);
    GPU_FinalizeDescriptorSet(lg->sweep_desc_set);
    return lg;
}

void PBR_DestroyLightgrid(PBR_Lightgrid* lg) {
    if (!lg) return;
    GPU_DestroyDescriptorSet(lg->sweep_desc_set);
    GPU_DestroyComputePipeline(lg->sweep_pipeline);                                      /* render.cpp:881 */
    GPU_DestroyPipelineLayout(lg->layout);
    GPU_DestroyTexture(lg->lightgrid);                                                   /* render.cpp:945 */
    free(lg);
}

GPU_Texture* PBR_LightgridTexture(PBR_Lightgrid* lg) { return lg->lightgrid; }
uint32_t PBR_LightgridSweepDirection(const PBR_Lightgrid* lg) { return lg->sweep_direction; }

void PBR_RecordLightgridClear(PBR_Lightgrid* lg, GPU_Graph* graph) {
    GPU_OpClearColorF(graph, lg->lightgrid, GPU_MIP_LEVEL_ALL, 0.f, 0.f, 0.f, 0.f);     /* render.cpp:1028 */
}

void PBR_RecordLightgridSweep(PBR_Lightgrid* lg, GPU_Graph* graph) {
    lg->sweep_direction++;                                                               /* render.cpp:1064-1065 */
    if (lg->sweep_direction == 3) lg->sweep_direction = 0;
    GPU_OpBindComputePipeline(graph, lg->sweep_pipeline);                                /* render.cpp:1067-1069 */
    GPU_OpBindComputeDescriptorSet(graph, lg->sweep_desc_set);
    GPU_OpPushComputeConstants(graph, lg->layout, &lg->sweep_direction, sizeof(lg->sweep_direction));
    /* render.cpp:1071-1072 asserts a 128^3 grid and dispatches (1,16,16) groups of 1x8x8; other cubic sizes scale the counts */
    uint32_t groups = lg->lightgrid->height / 8;
    GPU_OpDispatch(graph, 1, groups, groups);
}

void PBR_RecordLightgridSweepLines(PBR_Lightgrid* lg, GPU_Graph* graph, uint32_t direction, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1) {
    GPU_OpBindComputePipeline(graph, lg->sweep_pipeline);
    GPU_OpBindComputeDescriptorSet(graph, lg->sweep_desc_set);
    GPU_OpPushComputeConstants(graph, lg->layout, &direction, sizeof direction);
    GPUX_OpDispatchLines(graph, y0, y1, z0, z1);
}

/* ---- voxelise pass (K14) ---- */
struct PBR_VoxelizePass {
    PBR_Lightgrid* lightgrid;
    GPU_Texture* sun_depth_map;
    GPU_RenderPass* render_pass;
    GPU_PipelineLayout* layout;
    GPU_GraphicsPipeline* pipeline;
    GPU_Buffer* globals_buffer;
    GPU_Sampler* sampler_pcf;
    uint32_t binding[9];
    /* one descriptor set per (mesh, material) seen so far (the reference keeps one per part, asset_import.cpp:190-204) */
    const PBR_Mesh** set_mesh; PBR_Material** set_material; GPU_DescriptorSet** set; uint32_t set_count, set_cap;
};

PBR_VoxelizePass* PBR_MakeVoxelizePass(PBR_Lightgrid* lg, PBR_SunDepthPass* sun) {
    if (!lg || !sun) return NULL;
    PBR_VoxelizePass* p = (PBR_VoxelizePass*)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->lightgrid = lg; p->sun_depth_map = PBR_SunDepthTexture(sun);
    p->globals_buffer = GPU_MakeBuffer((uint32_t)sizeof(PBR_Globals) + 8, GPU_BufferFlag_CPU | GPU_BufferFlag_GPU | GPU_BufferFlag_StorageBuffer, NULL);
    /* render.cpp:664-673 */
    GPU_SamplerDesc pcf; memset(&pcf, 0, sizeof pcf);
    pcf.min_filter = pcf.mag_filter = pcf.mipmap_mode = GPU_Filter_Linear;
    pcf.address_modes[0] = pcf.address_modes[1] = pcf.address_modes[2] = GPU_AddressMode_Clamp;
    pcf.max_lod = 1000.f; pcf.compare_op = GPU_CompareOp_Less;
    p->sampler_pcf = GPU_MakeSampler(&pcf);
    /* render.cpp:711-714 */
    GPU_RenderPassDesc pass_desc; memset(&pass_desc, 0, sizeof pass_desc);
    pass_desc.width = lg->lightgrid->width; pass_desc.height = lg->lightgrid->width;
    p->render_pass = GPU_MakeRenderPass(&pass_desc);
    /* the bindings of the main pass layout that the shader reads (lightgrid_voxelize.glsl:22-30, 81-87) */
    p->layout = GPU_InitPipelineLayout();
    p->binding[0] = GPU_BufferBinding(p->layout, "GLOBALS");
    p->binding[1] = GPU_BufferBinding(p->layout, "SSBO0");
    p->binding[2] = GPU_BufferBinding(p->layout, "SSBO1");
    p->binding[3] = GPU_StorageImageBinding(p->layout, "IMG0", lg->lightgrid->format);
    p->binding[4] = GPU_TextureBinding(p->layout, "SUN_DEPTH_MAP");
    p->binding[5] = GPU_TextureBinding(p->layout, "TEX0");
    p->binding[6] = GPU_TextureBinding(p->layout, "TEX_EMISSIVE");
    p->binding[7] = GPU_SamplerBinding(p->layout, "SAMPLER_PERCENTAGE_CLOSER");
    p->binding[8] = GPU_SamplerBinding(p->layout, "SAMPLER_LINEAR_WRAP");
    GPU_FinalizePipelineLayout(p->layout);
    /* render.cpp:113-149 */
    static const char path[] = "../src/demo_pbr_renderer/shaders/lightgrid_voxelize.glsl";
    GPU_GraphicsPipelineDesc desc; memset(&desc, 0, sizeof desc);
    desc.layout = p->layout; desc.render_pass = p->render_pass;
    desc.vs.glsl_debug_filepath.data = path; desc.vs.glsl_debug_filepath.length = sizeof path - 1;
    desc.fs.glsl_debug_filepath = desc.vs.glsl_debug_filepath;
    GPU_GLSLErrorArray errors = {0};
    desc.vs.spirv = GPU_SPIRVFromGLSL(NULL, GPU_ShaderStage_Vertex, p->layout, &desc.vs, &errors);
    desc.fs.spirv = GPU_SPIRVFromGLSL(NULL, GPU_ShaderStage_Fragment, p->layout, &desc.fs, &errors);
    desc.enable_conservative_rasterization = true;
    desc.cull_mode = GPU_CullMode_TwoSided;
    p->pipeline = p->render_pass ? GPU_MakeGraphicsPipeline(&desc) : NULL;
    if (!p->globals_buffer || !p->sampler_pcf || !p->render_pass || !p->pipeline) { PBR_DestroyVoxelizePass(p); return NULL; }
    return p;
}

void PBR_DestroyVoxelizePass(PBR_VoxelizePass* p) {
    if (!p) return;
    for (uint32_t i = 0; i < p->set_count; ++i) GPU_DestroyDescriptorSet(p->set[i]);
    free(p->set); free(p->set_material); free((void*)p->set_mesh);
    GPU_DestroyGraphicsPipeline(p->pipeline);
    GPU_DestroyRenderPass(p->render_pass);
    GPU_DestroyPipelineLayout(p->layout);
    GPU_DestroySampler(p->sampler_pcf);
    GPU_DestroyBuffer(p->globals_buffer);
    free(p);
}

GPU_Buffer* PBR_VoxelizeGlobalsBuffer(PBR_VoxelizePass* p) { return p->globals_buffer; }
GPU_GraphicsPipeline* PBR_VoxelizePipeline(PBR_VoxelizePass* p) { return p->pipeline; }
GPU_RenderPass* PBR_VoxelizeRenderPass(PBR_VoxelizePass* p) { return p->render_pass; }
GPU_PipelineLayout* PBR_VoxelizeLayout(PBR_VoxelizePass* p) { return p->layout; }
GPU_Sampler* PBR_VoxelizeShadowSampler(PBR_VoxelizePass* p) { return p->sampler_pcf; }

GPU_DescriptorSet* PBR_VoxelizeDescriptorSet(PBR_VoxelizePass* p, const PBR_Mesh* mesh, PBR_Material* material) {
    if (!mesh || !material) return NULL;
    for (uint32_t i = 0; i < p->set_count; ++i) if (p->set_mesh[i] == mesh && p->set_material[i] == material) return p->set[i];
    if (p->set_count == p->set_cap) {
        uint32_t cap = p->set_cap ? 2 * p->set_cap : 16;
        const PBR_Mesh** sm = (const PBR_Mesh**)realloc((void*)p->set_mesh, cap * sizeof *sm);
        if (!sm) return NULL;
        p->set_mesh = sm;
        PBR_Material** sa = (PBR_Material**)realloc(p->set_material, cap * sizeof *sa);
        if (!sa) return NULL;
        p->set_material = sa;
        GPU_DescriptorSet** ss = (GPU_DescriptorSet**)realloc(p->set, cap * sizeof *ss);
        if (!ss) return NULL;
        p->set = ss; p->set_cap = cap;
    }
    /* asset_import.cpp:190-204 */
    GPU_DescriptorSet* s = GPU_InitDescriptorSet(NULL, p->layout);
    GPU_SetBufferBinding(s, p->binding[0], p->globals_buffer);
    GPU_SetBufferBinding(s, p->binding[1], mesh->vertex_buffer);
    GPU_SetBufferBinding(s, p->binding[2], mesh->index_buffer);
    GPU_SetStorageImageBinding(s, p->binding[3], p->lightgrid->lightgrid, 0);
    GPU_SetTextureBinding(s, p->binding[4], p->sun_depth_map);
    GPU_SetTextureBinding(s, p->binding[5], PBR_MaterialTexture(material, 0));
    GPU_SetTextureBinding(s, p->binding[6], PBR_MaterialTexture(material, 3));
    GPU_SetSamplerBinding(s, p->binding[7], p->sampler_pcf);
    GPU_SetSamplerBinding(s, p->binding[8], GPU_SamplerLinearWrap());
    GPU_FinalizeDescriptorSet(s);
    p->set_mesh[p->set_count] = mesh; p->set_material[p->set_count] = material; p->set[p->set_count] = s; p->set_count++;
    return s;
}

void PBR_RecordVoxelizePass(PBR_VoxelizePass* p, GPU_Graph* graph, const PBR_Mesh* mesh, const PBR_Globals* globals) {
    if (globals) memcpy(p->globals_buffer->data, globals, sizeof *globals);           /* render.cpp:991 */
    uint32_t* params = (uint32_t*)malloc((mesh->part_count ? mesh->part_count : 1) * sizeof *params);
    if (!params) return;
    GPU_OpPrepareRenderPass(graph, p->render_pass);                                     /* render.cpp:1039 */
    for (uint32_t i = 0; i < mesh->part_count; ++i) {                                   /* render.cpp:1041-1046 */
        GPU_DescriptorSet* s = PBR_VoxelizeDescriptorSet(p, mesh, mesh->materials[i]);
        params[i] = s ? GPU_OpPrepareDrawParams(graph, p->pipeline, s) : 0xFFFFFFFFu;
    }
    GPU_OpBeginRenderPass(graph);
    for (uint32_t i = 0; i < mesh->part_count; ++i) {                                   /* render.cpp:1050-1054 */
        if (params[i] == 0xFFFFFFFFu) continue;                                         /* a part without a material is not drawn */
        GPU_OpBindDrawParams(graph, params[i]);
        GPU_OpDraw(graph, mesh->parts[i].index_count, 1, mesh->parts[i].first_index, 0);
    }
    GPU_OpEndRenderPass(graph);
    free(params);
}
