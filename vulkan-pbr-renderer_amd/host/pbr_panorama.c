/*
 * pbr_panorama.c -- the bake's levels as lat-long panoramas (K20): the one image every HDRI viewer, DCC tool and image
 * diff opens.  The reference renderer writes no image at all; the strip writer of pbr_hdrio.c and the .dds writer of pbr_ddsout.c stay
 * what they are.  Contract of the mapping: csrc/panorama_core.h.
 */
#include "pbr_host.h"

#include <stdio.h>

static int is_f4_cube(const GPU_Texture* t, uint32_t mip) {
    return t && mip < t->mip_level_count && t->format == GPU_Format_RGBA32F && (t->flags & GPU_TextureFlag_Cubemap) && t->width == t->height;
}

GPU_Texture* PBR_MakePanoramaFromCube(GPU_Texture* cube, uint32_t mip_level, uint32_t width, uint32_t height, GPU_Format format) {
    if (!is_f4_cube(cube, mip_level)) { fprintf(stderr, "GPU-ERROR: PBR_MakePanoramaFromCube: the source must be a level of a square RGBA32F cubemap\n"); return NULL; }
    if (format != GPU_Format_RGBA32F && format != GPU_Format_RGBA16F) { fprintf(stderr, "GPU-ERROR: PBR_MakePanoramaFromCube: the target format must be RGBA32F or RGBA16F\n"); return NULL; }
    uint32_t n = cube->width >> mip_level; if (n < 1) n = 1;
    if (width == 0) width = 4 * n;
    if (height == 0) height = width / 2 ? width / 2 : 1;
    if (n > 16384 || width > 16384 || height > 16384) { fprintf(stderr, "GPU-ERROR: PBR_MakePanoramaFromCube: extents above 16384 are not implemented\n"); return NULL; }
    GPU_Texture* pano = GPU_MakeTexture(format, width, height, 1, 0, NULL);
    GPU_Graph* graph = pano ? GPU_MakeGraph() : NULL;
    if (!graph) { if (pano) GPU_DestroyTexture(pano); return NULL; }
    GPUX_OpCubeToPanorama(graph, cube, mip_level, pano, 0);
    GPU_GraphSubmit(graph);
    GPU_GraphWait(graph);
    GPU_DestroyGraph(graph);
    return pano;
}

int PBR_WritePanoramaHDR(const char* filepath, GPU_Texture* cube, uint32_t mip_level, uint32_t width, uint32_t height) {
    if (!filepath) return 1;
    GPU_Texture* pano = PBR_MakePanoramaFromCube(cube, mip_level, width, height, GPU_Format_RGBA32F);
    if (!pano) return 1;
    int rc = 2;
    const uint64_t bytes = GPUX_TextureMipBytes(pano, 0);
    GPU_Buffer* buf = bytes <= 0xFFFFFFFFu ? GPU_MakeBuffer((uint32_t)bytes, GPU_BufferFlag_CPU, NULL) : NULL;   /* a buffer holds < 4 GiB */
    GPU_Graph* graph = buf ? GPU_MakeGraph() : NULL;
    if (graph) {
        GPUX_OpCopyTextureMipToBuffer(graph, pano, 0, buf, 0);
        GPU_GraphSubmit(graph);
        GPU_GraphWait(graph);
        rc = PBR_WriteHDRFile(filepath, (const float*)buf->data, (int)pano->width, (int)pano->height);
        GPU_DestroyGraph(graph);
    }
    if (buf) GPU_DestroyBuffer(buf);
    GPU_DestroyTexture(pano);
    return rc;
}
