/*
 * pbr_geometry.c -- host side of the geometry pass (C11): materials and the reference renderer's geometry-pass objects and draw
 * sequence, restated against gpu_hip.h.
 *
 *   render.cpp:190-233             geometry pipelines (geometry_pass.glsl; depth test + write, GPU_CullMode_DrawCCW), one per velocity target
 *   render.cpp:680-691, :700-708   G-buffer targets and the two render passes (five colour targets + depth)
 *   render.cpp:993, :1076-1115     clear of the depth, PrepareRenderPass, PrepareDrawParams per part, BeginRenderPass, bind buffers,
 *                                  push the jitter pair, BindDrawParams + DrawIndexed per part, the skybox with its own buffers, EndRenderPass
 * The backend rasterises the pass with K13.
 */
#include "pbr_host.h"
#include "pbr_mesh.h"

#include <stdlib.h>
#include <string.h>

struct PBR_Material { GPU_Texture* tex[4]; bool owned[4]; };

PBR_Material* PBR_MakeMaterial(uint32_t size, const void* base_color, const void* normal, const void* orm, const void* emissive) {
    if (!size || (size & (size - 1)) || !base_color || !normal || !orm || !emissive) return NULL;
    PBR_Material* m = (PBR_Material*)calloc(1, sizeof *m);
    if (!m) return NULL;
    const void* src[4] = {base_color, normal, orm, emissive};
    for (int i = 0; i < 4; ++i) {
        m->tex[i] = GPU_MakeTexture(GPU_Format_RGBA8UN, size, size, 1, GPU_TextureFlag_HasMipmaps, src[i]);
        if (!m->tex[i]) { PBR_DestroyMaterial(m); return NULL; }
        m->owned[i] = true;
    }
    return m;
}

PBR_Material* PBR_MakeMaterialFromTextures(GPU_Texture* const tex[4]) {
    if (!tex) return NULL;
    PBR_Material* m = (PBR_Material*)calloc(1, sizeof *m);
    if (!m) return NULL;
    /* render.cpp:787-793: dummy_white, dummy_normal_map, dummy_black, dummy_black */
    static const uint32_t dummy[4] = {0xFFFFFFFFu, 0xFFFF7F7Fu, 0x00000000u, 0x00000000u};
    for (int i = 0; i < 4; ++i) {
        if (tex[i]) { m->tex[i] = tex[i]; continue; }
        m->tex[i] = GPU_MakeTexture(GPU_Format_RGBA8UN, 1, 1, 1, 0, &dummy[i]);
        if (!m->tex[i]) { PBR_DestroyMaterial(m); return NULL; }
        m->owned[i] = true;
    }
    return m;
}

void PBR_DestroyMaterial(PBR_Material* m) {
    if (!m) return;
    for (int i = 0; i < 4; ++i) if (m->owned[i]) GPU_DestroyTexture(m->tex[i]);
    free(m);
}

GPU_Texture* PBR_MaterialTexture(PBR_Material* m, uint32_t which) { return which < 4 ? m->tex[which] : NULL; }

struct PBR_GeometryPass {
    GPU_RenderPass* render_pass[2];
    GPU_GraphicsPipeline* pipeline[2];
    GPU_PipelineLayout* layout;
    GPU_Buffer* globals_buffer;
    GPU_Texture* depth;
    uint32_t binding[6];
    /* one descriptor set per material seen so far (the reference keeps one per part, render.cpp:1081) */
    PBR_Material** set_material; GPU_DescriptorSet** set; uint32_t set_count, set_cap;
};

PBR_GeometryPass* PBR_MakeGeometryPass(const PBR_GBuffer* gb, PBR_PostProcess* pp, uint32_t width, uint32_t height) {
    if (!gb || !pp) return NULL;
    PBR_GeometryPass* p = (PBR_GeometryPass*)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->globals_buffer = GPU_MakeBuffer((uint32_t)sizeof(PBR_Globals) + 8, GPU_BufferFlag_CPU | GPU_BufferFlag_GPU | GPU_BufferFlag_StorageBuffer, NULL);
    p->depth = gb->depth;
    p->layout = GPU_InitPipelineLayout();
    p->binding[0] = GPU_BufferBinding(p->layout, "GLOBALS");
    p->binding[1] = GPU_TextureBinding(p->layout, "TEX0");
    p->binding[2] = GPU_TextureBinding(p->layout, "TEX1");
    p->binding[3] = GPU_TextureBinding(p->layout, "TEX_ORM");
    p->binding[4] = GPU_TextureBinding(p->layout, "TEX_EMISSIVE");
    p->binding[5] = GPU_SamplerBinding(p->layout, "SAMPLER_LINEAR_WRAP");
    GPU_FinalizePipelineLayout(p->layout);
    static const char path[] = "../src/demo_pbr_renderer/shaders/geometry_pass.glsl";
    for (int i = 0; i < 2; ++i) {
        /* render.cpp:700-708 */
        GPU_TextureView targets[5] = {{gb->base_color, 0}, {gb->normal, 0}, {gb->orm, 0}, {gb->emissive, 0}, {PBR_PostVelocity(pp, (uint32_t)i), 0}};
        GPU_RenderPassDesc pass_desc; memset(&pass_desc, 0, sizeof pass_desc);
        pass_desc.width = width; pass_desc.height = height;
        pass_desc.color_targets = targets; pass_desc.color_targets_count = 5;
        pass_desc.depth_stencil_target = gb->depth;
        p->render_pass[i] = GPU_MakeRenderPass(&pass_desc);
        /* render.cpp:190-233 */
        GPU_GraphicsPipelineDesc desc; memset(&desc, 0, sizeof desc);
        desc.layout = p->layout; desc.render_pass = p->render_pass[i];
        desc.vs.glsl_debug_filepath.data = path; desc.vs.glsl_debug_filepath.length = sizeof path - 1;
        desc.fs.glsl_debug_filepath = desc.vs.glsl_debug_filepath;
        GPU_GLSLErrorArray errors = {0};
        desc.vs.spirv = GPU_SPIRVFromGLSL(NULL, GPU_ShaderStage_Vertex, p->layout, &desc.vs, &errors);
        desc.fs.spirv = GPU_SPIRVFromGLSL(NULL, GPU_ShaderStage_Fragment, p->layout, &desc.fs, &errors);
        GPU_Format vertex_formats[] = {GPU_Format_RGB32F, GPU_Format_RGB32F, GPU_Format_RGB32F, GPU_Format_RG32F};
        desc.vertex_input_formats = vertex_formats; desc.vertex_input_formats_count = 4;
        desc.enable_depth_test = true; desc.enable_depth_write = true;
        desc.cull_mode = GPU_CullMode_DrawCCW;
        p->pipeline[i] = p->render_pass[i] ? GPU_MakeGraphicsPipeline(&desc) : NULL;
    }
    if (!p->globals_buffer || !p->render_pass[0] || !p->render_pass[1] || !p->pipeline[0] || !p->pipeline[1]) { PBR_DestroyGeometryPass(p); return NULL; }
    return p;
}

void PBR_DestroyGeometryPass(PBR_GeometryPass* p) {
    if (!p) return;
    for (uint32_t i = 0; i < p->set_count; ++i) GPU_DestroyDescriptorSet(p->set[i]);
    free(p->set); free(p->set_material);
    for (int i = 0; i < 2; ++i) { GPU_DestroyGraphicsPipeline(p->pipeline[i]); GPU_DestroyRenderPass(p->render_pass[i]); }
    GPU_DestroyPipelineLayout(p->layout);
    GPU_DestroyBuffer(p->globals_buffer);
    free(p);
}

GPU_Buffer* PBR_GeometryGlobalsBuffer(PBR_GeometryPass* p) { return p->globals_buffer; }
GPU_GraphicsPipeline* PBR_GeometryPipeline(PBR_GeometryPass* p, uint32_t i) { return p->pipeline[i & 1]; }
GPU_RenderPass* PBR_GeometryRenderPass(PBR_GeometryPass* p, uint32_t i) { return p->render_pass[i & 1]; }
GPU_PipelineLayout* PBR_GeometryLayout(PBR_GeometryPass* p) { return p->layout; }

GPU_DescriptorSet* PBR_GeometryDescriptorSet(PBR_GeometryPass* p, PBR_Material* material) {
    if (!material) return NULL;
    for (uint32_t i = 0; i < p->set_count; ++i) if (p->set_material[i] == material) return p->set[i];
    if (p->set_count == p->set_cap) {
        uint32_t cap = p->set_cap ? 2 * p->set_cap : 16;
        PBR_Material** sm = (PBR_Material**)realloc(p->set_material, cap * sizeof *sm);
        if (!sm) return NULL;
        p->set_material = sm;
        GPU_DescriptorSet** ss = (GPU_DescriptorSet**)realloc(p->set, cap * sizeof *ss);
        if (!ss) return NULL;
        p->set = ss; p->set_cap = cap;
    }
    GPU_DescriptorSet* s = GPU_InitDescriptorSet(NULL, p->layout);
    GPU_SetBufferBinding(s, p->binding[0], p->globals_buffer);
    for (uint32_t k = 0; k < 4; ++k) GPU_SetTextureBinding(s, p->binding[1 + k], material->tex[k]);
    GPU_SetSamplerBinding(s, p->binding[5], GPU_SamplerLinearWrap());
    GPU_FinalizeDescriptorSet(s);
    p->set_material[p->set_count] = material; p->set[p->set_count] = s; p->set_count++;
    return s;
}

void PBR_RecordGeometryPass(PBR_GeometryPass* p, GPU_Graph* graph, const PBR_Mesh* mesh, const PBR_Mesh* skybox, const PBR_Globals* globals,
                            const float* jitter, const float* jitter_prev, uint32_t frame_idx) {
    const uint32_t f = frame_idx & 1;
    if (globals) memcpy(p->globals_buffer->data, globals, sizeof *globals);           /* render.cpp:991 */
    GPU_OpClearDepthStencil(graph, p->depth, GPU_MIP_LEVEL_ALL);      /* render.cpp:993 */
    const PBR_Mesh* meshes[2] = {mesh, skybox};
    uint32_t total = mesh->part_count + (skybox ? skybox->part_count : 0);
    uint32_t* params = (uint32_t*)malloc((total ? total : 1) * sizeof *params);
    if (!params) return;
    GPU_OpPrepareRenderPass(graph, p->render_pass[f]);
    uint32_t n = 0;
    for (int k = 0; k < 2; ++k) {                                                      /* render.cpp:1078-1083 */
        if (!meshes[k]) continue;
        for (uint32_t i = 0; i < meshes[k]->part_count; ++i) {
            GPU_DescriptorSet* s = PBR_GeometryDescriptorSet(p, meshes[k]->materials[i]);
            params[n++] = s ? GPU_OpPrepareDrawParams(graph, p->pipeline[f], s) : 0xFFFFFFFFu;
        }
    }
    GPU_OpBeginRenderPass(graph);
    float constants[4] = {jitter ? jitter[0] : 0.0f, jitter ? jitter[1] : 0.0f, jitter_prev ? jitter_prev[0] : 0.0f, jitter_prev ? jitter_prev[1] : 0.0f};
    n = 0;
    for (int k = 0; k < 2; ++k) {
        if (!meshes[k]) continue;
        GPU_OpBindVertexBuffer(graph, meshes[k]->vertex_buffer);                       /* render.cpp:1088-1089, :1105-1106 */
        GPU_OpBindIndexBuffer(graph, meshes[k]->index_buffer);
        if (k == 0) GPU_OpPushGraphicsConstants(graph, p->layout, constants, sizeof constants);   /* render.cpp:1091-1094 */
        for (uint32_t i = 0; i < meshes[k]->part_count; ++i, ++n) {
            if (params[n] == 0xFFFFFFFFu) continue;                                     /* a part without a material is not drawn */
            GPU_OpBindDrawParams(graph, params[n]);
            GPU_OpDrawIndexed(graph, meshes[k]->parts[i].index_count, 1, meshes[k]->parts[i].first_index, 0, 0);
        }
    }
    GPU_OpEndRenderPass(graph);
    free(params);
}
