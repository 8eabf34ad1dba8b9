/*
 * pbr_shadow.c -- host side of the sun shadow depth pass (C11): the merged scene buffers and the reference renderer's sun-depth
 * objects and draw sequence, restated against gpu_hip.h.
 *
 *   asset_import.cpp:172-173       one vertex buffer + one index buffer for the whole scene, parts = index ranges
 *   render.cpp:88-111              sun depth pipeline (sun_depth_pass.glsl; position, normal, tangent, tex_coord; depth test + write)
 *   render.cpp:677, :725-729       2048^2 D32F target, depth-only render pass
 *   render.cpp:995-1020            clear, PrepareRenderPass, PrepareDrawParams per part, BeginRenderPass, bind buffers,
 *                                  BindDrawParams + DrawIndexed per part, EndRenderPass
 * The backend rasterises the pass with K12; its texture is the SUN_DEPTH_MAP of the lighting pass.
 */
#include "pbr_host.h"
#include "pbr_mesh.h"

#include <stdlib.h>
#include <string.h>

PBR_Mesh* PBR_MakeMesh(const float* vertices_11f, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                       const PBR_MeshPart* parts, uint32_t part_count) {
    if (!vertices_11f || !vertex_count || !indices || !index_count || (part_count && !parts)) return NULL;
    if ((uint64_t)vertex_count * 44u > 0xFFFFFFFFu || (uint64_t)index_count * 4u > 0xFFFFFFFFu) return NULL;   /* GPU_MakeBuffer takes a uint32 size */
    PBR_Mesh* m = (PBR_Mesh*)calloc(1, sizeof *m);
    if (!m) return NULL;
    /* asset_import.cpp:172-173 */
    m->vertex_buffer = GPU_MakeBuffer(vertex_count * 44u, GPU_BufferFlag_GPU | GPU_BufferFlag_StorageBuffer, vertices_11f);
    m->index_buffer = GPU_MakeBuffer(index_count * 4u, GPU_BufferFlag_GPU | GPU_BufferFlag_StorageBuffer, indices);
    m->parts = (PBR_MeshPart*)malloc((part_count ? part_count : 1) * sizeof *m->parts);
    m->materials = (PBR_Material**)calloc(part_count ? part_count : 1, sizeof *m->materials);
    if (!m->vertex_buffer || !m->index_buffer || !m->parts || !m->materials) { PBR_DestroyMesh(m); return NULL; }
    if (part_count) memcpy(m->parts, parts, part_count * sizeof *parts);
    m->part_count = part_count;
    return m;
}

void PBR_DestroyMesh(PBR_Mesh* m) {
    if (!m) return;
    GPU_DestroyBuffer(m->vertex_buffer);
    GPU_DestroyBuffer(m->index_buffer);
    free(m->parts);
    free(m->materials);
    free(m);
}

GPU_Buffer* PBR_MeshVertexBuffer(PBR_Mesh* m) { return m->vertex_buffer; }
GPU_Buffer* PBR_MeshIndexBuffer(PBR_Mesh* m) { return m->index_buffer; }
uint32_t PBR_MeshPartCount(const PBR_Mesh* m) { return m->part_count; }
void PBR_MeshSetPartMaterial(PBR_Mesh* m, uint32_t part, PBR_Material* material) { if (part < m->part_count) m->materials[part] = material; }

struct PBR_SunDepthPass {
    GPU_Texture* sun_depth_rt;
    GPU_RenderPass* render_pass;
    GPU_PipelineLayout* layout;
    GPU_GraphicsPipeline* pipeline;
    GPU_DescriptorSet* desc_set;
    GPU_Buffer* globals_buffer;
};

PBR_SunDepthPass* PBR_MakeSunDepthPass(uint32_t size) {
    PBR_SunDepthPass* p = (PBR_SunDepthPass*)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->globals_buffer = GPU_MakeBuffer((uint32_t)sizeof(PBR_Globals) + 8, GPU_BufferFlag_CPU | GPU_BufferFlag_GPU | GPU_BufferFlag_StorageBuffer, NULL);
    /* render.cpp:677 */
    p->sun_depth_rt = GPU_MakeTexture(GPU_Format_D32F_Or_X8D24UN, size, size, 1, GPU_TextureFlag_RenderTarget, NULL);
    /* render.cpp:725-729 */
    GPU_RenderPassDesc pass_desc; memset(&pass_desc, 0, sizeof pass_desc);
    pass_desc.width = size; pass_desc.height = size;
    pass_desc.depth_stencil_target = p->sun_depth_rt;
    p->render_pass = GPU_MakeRenderPass(&pass_desc);
    /* the reference shares its main pass layout; the sun pass reads GLOBALS only (sun_depth_pass.glsl:23-25) */
    p->layout = GPU_InitPipelineLayout();
    uint32_t globals_b = GPU_BufferBinding(p->layout, "GLOBALS");
    GPU_FinalizePipelineLayout(p->layout);
    /* render.cpp:88-111 */
    static const char path[] = "../src/demo_pbr_renderer/shaders/sun_depth_pass.glsl";
    GPU_GraphicsPipelineDesc desc; memset(&desc, 0, sizeof desc);
    desc.layout = p->layout; desc.render_pass = p->render_pass;
    desc.vs.glsl_debug_filepath.data = path; desc.vs.glsl_debug_filepath.length = sizeof path - 1;
    desc.fs.glsl_debug_filepath = desc.vs.glsl_debug_filepath;
    GPU_GLSLErrorArray errors = {0};
    desc.vs.spirv = GPU_SPIRVFromGLSL(NULL, GPU_ShaderStage_Vertex, p->layout, &desc.vs, &errors);
    desc.fs.spirv = GPU_SPIRVFromGLSL(NULL, GPU_ShaderStage_Fragment, p->layout, &desc.fs, &errors);
    GPU_Format vertex_formats[] = {GPU_Format_RGB32F, GPU_Format_RGB32F, GPU_Format_RGB32F, GPU_Format_RG32F};
    desc.vertex_input_formats = vertex_formats; desc.vertex_input_formats_count = 4;
    desc.enable_depth_test = true; desc.enable_depth_write = true;
    desc.cull_mode = GPU_CullMode_TwoSided;
    p->pipeline = GPU_MakeGraphicsPipeline(&desc);
    p->desc_set = GPU_InitDescriptorSet(NULL, p->layout);
    GPU_SetBufferBinding(p->desc_set, globals_b, p->globals_buffer);
    GPU_FinalizeDescriptorSet(p->desc_set);
    if (!p->globals_buffer || !p->sun_depth_rt || !p->render_pass || !p->pipeline) { PBR_DestroySunDepthPass(p); return NULL; }
    return p;
}

void PBR_DestroySunDepthPass(PBR_SunDepthPass* p) {
    if (!p) return;
    GPU_DestroyDescriptorSet(p->desc_set);
    GPU_DestroyGraphicsPipeline(p->pipeline);
    GPU_DestroyPipelineLayout(p->layout);
    GPU_DestroyRenderPass(p->render_pass);
    GPU_DestroyTexture(p->sun_depth_rt);
    GPU_DestroyBuffer(p->globals_buffer);
    free(p);
}

GPU_Texture* PBR_SunDepthTexture(PBR_SunDepthPass* p) { return p->sun_depth_rt; }
GPU_Buffer* PBR_SunDepthGlobalsBuffer(PBR_SunDepthPass* p) { return p->globals_buffer; }
GPU_GraphicsPipeline* PBR_SunDepthPipeline(PBR_SunDepthPass* p) { return p->pipeline; }
GPU_RenderPass* PBR_SunDepthRenderPass(PBR_SunDepthPass* p) { return p->render_pass; }
GPU_PipelineLayout* PBR_SunDepthLayout(PBR_SunDepthPass* p) { return p->layout; }
GPU_DescriptorSet* PBR_SunDepthDescriptorSet(PBR_SunDepthPass* p) { return p->desc_set; }

void PBR_RecordSunDepthPass(PBR_SunDepthPass* p, GPU_Graph* graph, const PBR_Mesh* mesh, const PBR_Globals* globals) {
    if (globals) memcpy(p->globals_buffer->data, globals, sizeof *globals);           /* render.cpp:991 */
    GPU_OpClearDepthStencil(graph, p->sun_depth_rt, GPU_MIP_LEVEL_ALL);                 /* render.cpp:995 */
    GPU_OpPrepareRenderPass(graph, p->render_pass);
    /* render.cpp:999-1005: one draw-params entry per part (the reference passes each part's own set; they share GLOBALS) */
    uint32_t* params = (uint32_t*)malloc((mesh->part_count ? mesh->part_count : 1) * sizeof *params);
    if (!params) return;
    for (uint32_t i = 0; i < mesh->part_count; ++i) params[i] = GPU_OpPrepareDrawParams(graph, p->pipeline, p->desc_set);
    GPU_OpBeginRenderPass(graph);
    GPU_OpBindVertexBuffer(graph, mesh->vertex_buffer);
    GPU_OpBindIndexBuffer(graph, mesh->index_buffer);
    for (uint32_t i = 0; i < mesh->part_count; ++i) {                                   /* render.cpp:1012-1016 */
        GPU_OpBindDrawParams(graph, params[i]);
        GPU_OpDrawIndexed(graph, mesh->parts[i].index_count, 1, mesh->parts[i].first_index, 0, 0);
    }
    GPU_OpEndRenderPass(graph);
    free(params);
}
