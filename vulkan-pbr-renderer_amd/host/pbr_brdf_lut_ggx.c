/*
 * pbr_brdf_lut_ggx.c -- the split-sum BRDF LUT of the GGX lobe (K22; no reference counterpart: render.cpp:591-619
 * dispatches the Beckmann quadrature of K1): the LUT that goes with the specular map of PBR_GenPrefilteredEnvMapGGX, by
 * GPUX_OpBrdfLutGGX over all rows.  Contract of the op: csrc/brdf_lut_ggx_core.h.
 */
#include "pbr_host.h"

#include <stdio.h>

void PBR_GenBRDFIntegrationMapGGX(GPU_Texture* brdf_lut, uint32_t sample_count, uint32_t visibility) {
    if (!brdf_lut) { fprintf(stderr, "GPU-ERROR: PBR_GenBRDFIntegrationMapGGX: NULL texture\n"); return; }
    GPU_Graph* graph = GPU_MakeGraph();
    GPUX_OpBrdfLutGGX(graph, brdf_lut, sample_count, visibility, 0, brdf_lut->height);   /* checks the rest */
    GPU_GraphSubmit(graph);
    GPU_GraphWait(graph);
    GPU_DestroyGraph(graph);
}
