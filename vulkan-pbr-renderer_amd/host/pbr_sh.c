/*
 * pbr_sh.c -- the SH9 form of the environment's diffuse lighting (K17): what other IBL bakers emit as "the 27
 * numbers" (cmft, IBLBaker, cmgen --sh).  The reference renderer has no counterpart; its diffuse output is the cube of
 * gen_irradiance_map.glsl, which PBR_GenIrradianceMap keeps producing.  Contract: csrc/sh_core.h.
 */
#include "pbr_host.h"
#include "../csrc/sh_core.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int is_f4_cube(const GPU_Texture* t, uint32_t mip) {
    return t && mip < t->mip_level_count && t->format == GPU_Format_RGBA32F && (t->flags & GPU_TextureFlag_Cubemap) && t->width == t->height;
}
static uint32_t level_size(const GPU_Texture* t, uint32_t mip) { uint32_t n = t->width >> mip; return n ? n : 1; }

int PBR_ProjectSH9(GPU_Texture* cube, uint32_t mip_level, double out[27]) {
    if (!out || !is_f4_cube(cube, mip_level)) return 1;
    GPU_Buffer* buf = GPU_MakeBuffer(27 * sizeof(double), GPU_BufferFlag_CPU, NULL);
    GPU_Graph* graph = GPU_MakeGraph();
    if (!buf || !graph) { if (graph) GPU_DestroyGraph(graph); GPU_DestroyBuffer(buf); return 1; }
    GPUX_OpProjectSH9(graph, cube, mip_level, 0, 6, 0, level_size(cube, mip_level), buf, 0);
    GPU_GraphSubmit(graph);
    GPU_GraphWait(graph);
    memcpy(out, buf->data, 27 * sizeof(double));
    GPU_DestroyGraph(graph);
    GPU_DestroyBuffer(buf);
    return 0;
}

void PBR_GenIrradianceMapSH(GPU_Texture* tex_env_cube, uint32_t src_mip_level, GPU_Texture* irradiance_map) {
    if (!is_f4_cube(tex_env_cube, src_mip_level) || !irradiance_map) return;
    GPU_Buffer* coef = GPU_MakeBuffer(27 * sizeof(double), GPU_BufferFlag_GPU, NULL);
    GPU_Graph* graph = GPU_MakeGraph();
    if (coef && graph) {
        GPUX_OpProjectSH9(graph, tex_env_cube, src_mip_level, 0, 6, 0, level_size(tex_env_cube, src_mip_level), coef, 0);
        GPUX_OpIrradianceFromSH9(graph, coef, 0, irradiance_map, 0);
        GPU_GraphSubmit(graph);
        GPU_GraphWait(graph);
    }
    if (graph) GPU_DestroyGraph(graph);
    GPU_DestroyBuffer(coef);
}

/* n need not have unit length: it is normalised in double */
void PBR_EvalSH9Irradiance(const double coef[27], const float n[3], float rgb[3]) {
    const double x = n[0], y = n[1], z = n[2], inv = 1.0 / sqrt((x * x + y * y) + z * z);
    const double d[3] = {x * inv, y * inv, z * inv};
    double e[3];
    sh_irradiance(coef, d, e);
    for (int c = 0; c < 3; ++c) rgb[c] = (float)e[c];
}

#define SH9_FILE_HEADER "# SH9 radiance coefficients, RGB per line, order L00 L1-1(y) L10(z) L11(x) L2-2(xy) L2-1(yz) L20(3zz-1) L21(xz) L22(xx-yy); " \
                        "real orthonormal basis, no Condon-Shortley phase; irradiance/(2 pi) = sum a_k c_k Y_k, a = 1/2 1/3 1/3 1/3 1/8 1/8 1/8 1/8 1/8"

int PBR_WriteSH9File(const char* path, const double coef[27]) {
    FILE* f = path && coef ? fopen(path, "w") : NULL;
    if (!f) return 1;
    int ok = fprintf(f, "%s\n", SH9_FILE_HEADER) > 0;
    for (int k = 0; k < 9 && ok; ++k) ok = fprintf(f, "%.17g %.17g %.17g\n", coef[3 * k], coef[3 * k + 1], coef[3 * k + 2]) > 0;
    if (fclose(f) != 0) ok = 0;
    return ok ? 0 : 1;
}

/* strict: one '#' line, then exactly nine lines of three numbers and nothing else */
int PBR_ReadSH9File(const char* path, double coef[27]) {
    FILE* f = path && coef ? fopen(path, "r") : NULL;
    if (!f) return 1;
    char line[1024];
    double v[27];
    int ok = fgets(line, sizeof line, f) && line[0] == '#' && strchr(line, '\n');
    for (int k = 0; k < 9 && ok; ++k) {
        ok = fgets(line, sizeof line, f) && strchr(line, '\n');
        char* p = line;
        for (int c = 0; c < 3 && ok; ++c) {
            char* end = NULL;
            errno = 0;
            v[3 * k + c] = strtod(p, &end);
            ok = end != p && (*end == ' ' || *end == '\n') && (c == 2) == (*end == '\n');
            p = end + 1;
        }
    }
    if (ok && fgets(line, sizeof line, f)) ok = 0;                              /* anything after the ninth line */
    fclose(f);
    if (!ok) return 1;
    memcpy(coef, v, sizeof v);
    return 0;
}
