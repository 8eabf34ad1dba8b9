/*
 * pbr_prefilter_ggx.c -- the specular map baked the way the lighting pass reads it (K21; no reference counterpart):
 * level 0 as PBR_GenPrefilteredEnvMap records it, the levels below by GPUX_OpPrefilterGGX at roughness min(1, i / 4), the value
 * lighting_pass.glsl:699 assumes when it fetches lod = roughness * 4.  Contract of the op: csrc/prefilter_ggx_core.h.
 */
#include "pbr_host.h"

#include <stdio.h>

void PBR_GenPrefilteredEnvMapGGX(GPU_Texture* tex_env_cube, GPU_Texture* spec, uint32_t min_size, uint32_t sample_count) {
    if (!tex_env_cube || !spec) { fprintf(stderr, "GPU-ERROR: PBR_GenPrefilteredEnvMapGGX: NULL texture\n"); return; }
    if (sample_count < 1 || sample_count > 4096) { fprintf(stderr, "GPU-ERROR: PBR_GenPrefilteredEnvMapGGX: %u samples outside 1 .. 4096\n", sample_count); return; }
    PBR_IBLPipelines* p = PBR_MakeIBLPipelines();
    GPU_Graph* graph = GPU_MakeGraph();
    GPU_DescriptorArena* descriptor_arena = GPU_MakeDescriptorArena();

    uint32_t size = spec->width;
    for (uint32_t i = 0; i < spec->mip_level_count; i++) {
        if (size < min_size) break;
        if (i == 0) PBR_RecordPrefilterLevel(p, graph, descriptor_arena, tex_env_cube, spec, 0);
        else GPUX_OpPrefilterGGX(graph, tex_env_cube, spec, i, i < 4 ? (float)i / 4.0f : 1.0f, sample_count, 1.0f, 0, 6, 0, size);
        size /= 2;
    }
    GPU_GraphSubmit(graph);
    GPU_GraphWait(graph);

    GPU_DestroyDescriptorArena(descriptor_arena);
    GPU_DestroyGraph(graph);
    PBR_DestroyIBLPipelines(p);
}
