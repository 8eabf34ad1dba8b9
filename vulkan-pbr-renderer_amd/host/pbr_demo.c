/*
 * pbr_demo.c -- headless C driver of the hot path through the GPU_* boundary (what main.cpp:35-51 +
 * HotreloadShaders + BuildRenderCommands do for this path, without window / mesh import / raster passes).
 *
 *   pbr_demo <cube_strip.hdr> [irradiance_size lut_size specular_size min_size [width height [frame.ppm [raster [gridview]]]]] [sh9 FILE] [dds|dds2 PREFIX] [ddsin PREFIX] [sh9shade] [pano PREFIX] [ggx N | ggxpair N]
 *
 * Loads a vertical-strip HDR cube (asset_import.cpp:17-27), runs the IBL precompute (render.cpp:505-619),
 * shades a flat synthetic G-buffer (a metallic floor under the sky), then runs three frames of the per-frame chain
 * lighting -> TAA resolve -> bloom -> tone map (render.cpp:1119-1187) plus the light-grid sweep (render.cpp:1061-1072),
 * and prints fp64 checksums of every map / frame plus HIP-event timings per kernel, one "key value" pair per line, so
 * that a test can compare it with the same sequence driven from another language.  With a last argument the 8-bit
 * frame is written as a binary PPM.  With `raster` as the ninth argument the three frames of the chain start with the geometry pass
 * (render.cpp:1076-1115) over a small built-in mesh (a checkered floor and a block), so the lighting pass shades a rasterised
 * G-buffer instead of the synthetic one, and the light grid's lit voxels are not a stand-in either: the sun depth pass and the
 * voxelise pass (render.cpp:995-1020, 1039-1056) draw that mesh into it; every other output is unchanged.  With `gridview` as the
 * tenth argument (after `raster`) one more frame is rendered with Globals.visualize_lightgrid set -- the reference's G key, kernel
 * K16: the voxelised mesh itself -- and its checksum is printed as gridview_bits_sum; the other lines stay as they are.
 * With `sh9 FILE` as the LAST two arguments (after whichever of the above are given) the SH9 coefficients of level 0 of the loaded
 * environment (K17) are written to FILE and their sum is printed as sh9_sum; the other lines stay as they are.
 * With `dds PREFIX` as the last two arguments (after `sh9 FILE` if both are given) the bake is saved as PREFIX_specular.dds (BC6H_UF16
 * through K18, the levels down to min_size), PREFIX_irradiance.dds and PREFIX_lut.dds (as they are), and the three file sizes are
 * printed as dds_bytes; the other lines stay as they are.  `dds2 PREFIX` in the same place writes the same three files with the
 * specular cube encoded at K18's two-region quality (PBR_DDS_OUT_BC6H_UF16_2R).
 * With `ddsin PREFIX` as the last two arguments (after all of the above) nothing is baked: the three maps are loaded from
 * PREFIX_specular.dds (a BC6H_UF16 file is decoded by K19 into an RGBA32F cube, a float file is loaded as it is), PREFIX_irradiance.dds
 * and PREFIX_lut.dds -- the files `dds PREFIX` wrote -- and the run goes on unchanged from the irradiance_sum line.
 * With `sh9shade` as the LAST argument (after all of the above) the first frame is rendered once more with the ambient term taken from
 * the SH9 coefficients of level 0 of the environment instead of the irradiance cube (K17's projection and K5 in SH9 mode in one
 * graph, PBR_LightingUseSH9), and its checksum is printed as frame_sh9_checksum; the other lines stay as they are.
 * With `pano PREFIX` as the LAST two arguments (after all of the above, `sh9shade` included) the baked maps are also written as lat-long
 * panoramas one can look at (K20, PBR_WritePanoramaHDR at the default extent 4 n x 2 n): PREFIX_irradiance.hdr and PREFIX_specular_mipN.hdr
 * for every level that has a specular_mipN_sum line, and each file's extent is printed as pano_extent; the other lines stay as they are.
 * With `ggx N` as the LAST two arguments (after all of the above, `pano PREFIX` included) the specular map is baked by K21
 * (PBR_GenPrefilteredEnvMapGGX, N samples per texel): level 0 is the same copy, the levels below it are the GGX prefilter at the
 * roughness the lighting pass reads them at.  Every line keeps its name; specular_mip0_sum keeps its value.
 * With `ggxpair N` in the same place the specular map is baked the same way and the BRDF LUT is its split-sum partner, K22's GGX LUT
 * (PBR_GenBRDFIntegrationMapGGX, N samples per texel, the Smith-Schlick term the lighting pass evaluates), in place of K1's Beckmann
 * LUT: against `ggx N` only lut_bits_sum and what is shaded with the LUT change.
 */
#include "pbr_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static double checksum_texture_mip(GPU_Texture* tex, uint32_t mip, int channels_f32) {
    uint64_t bytes = GPUX_TextureMipBytes(tex, mip);
    GPU_Buffer* buf = GPU_MakeBuffer((uint32_t)bytes, GPU_BufferFlag_CPU, NULL);
    GPU_Graph* g = GPU_MakeGraph();
    GPUX_OpCopyTextureMipToBuffer(g, tex, mip, buf, 0);
    GPU_GraphSubmit(g);
    GPU_GraphWait(g);
    double sum = 0.0;
    if (channels_f32) {
        const float* f = (const float*)buf->data;
        for (uint64_t i = 0; i < bytes / 4; ++i) sum += (double)f[i];
    } else {
        const uint16_t* h = (const uint16_t*)buf->data;           /* fp16 payloads: checksum of the raw bit patterns */
        for (uint64_t i = 0; i < bytes / 2; ++i) sum += (double)h[i];
    }
    GPU_DestroyGraph(g);
    GPU_DestroyBuffer(buf);
    return sum;
}

/* opt-in `raster` mode: a two-sided floor and block, one procedural material */
static PBR_Mesh* demo_mesh(PBR_Material** material_out) {
    enum { S = 16 };
    static uint8_t img[4][S * S * 4];
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            const int on = ((x >> 2) + (y >> 2)) & 1;
            uint8_t* b = img[0] + 4 * (y * S + x); b[0] = on ? 230 : 90; b[1] = on ? 200 : 80; b[2] = on ? 120 : 70; b[3] = 255;
            uint8_t* n = img[1] + 4 * (y * S + x); n[0] = 128; n[1] = 128; n[2] = 255; n[3] = 255;
            uint8_t* o = img[2] + 4 * (y * S + x); o[0] = 255; o[1] = on ? 60 : 160; o[2] = on ? 255 : 0; o[3] = 255;
            uint8_t* e = img[3] + 4 * (y * S + x); e[0] = 0; e[1] = 0; e[2] = 0; e[3] = 255;
        }
    *material_out = PBR_MakeMaterial(S, img[0], img[1], img[2], img[3]);
    /* quads as (corner, edge u, edge v, normal); each drawn with both windings */
    static const float quads[3][12] = {
        {-40.f, 2.f, 0.f, 80.f, 0.f, 0.f, 0.f, 80.f, 0.f, 0.f, 0.f, 1.f},       /* floor z = 0 */
        {-3.f, 14.f, 0.f, 6.f, 0.f, 0.f, 0.f, 0.f, 6.f, 0.f, -1.f, 0.f},        /* block front */
        {-3.f, 14.f, 6.f, 6.f, 0.f, 0.f, 0.f, 6.f, 0.f, 0.f, 0.f, 1.f}};        /* block top */
    float v[3 * 4 * 11]; uint32_t ix[3 * 12]; uint32_t nv = 0, ni = 0;
    for (int q = 0; q < 3; ++q) {
        const float* Q = quads[q];
        for (int c = 0; c < 4; ++c) {
            const float a = (c == 1 || c == 2) ? 1.f : 0.f, b = c >= 2 ? 1.f : 0.f;
            float* o = v + 11 * (nv + c);
            for (int e = 0; e < 3; ++e) { o[e] = Q[e] + a * Q[3 + e] + b * Q[6 + e]; o[3 + e] = Q[9 + e]; o[6 + e] = e == 0 ? 1.f : 0.f; }
            o[9] = a * (q == 0 ? 20.f : 2.f); o[10] = b * (q == 0 ? 20.f : 2.f);
        }
        const uint32_t t[12] = {0, 1, 2, 0, 2, 3, 0, 2, 1, 0, 3, 2};
        for (int k = 0; k < 12; ++k) ix[ni++] = nv + t[k];
        nv += 4;
    }
    PBR_MeshPart part = {0, ni};
    PBR_Mesh* m = PBR_MakeMesh(v, nv, ix, ni, &part, 1);
    if (m) PBR_MeshSetPartMaterial(m, 0, *material_out);
    return m;
}

/* `ddsin PREFIX`: the bake's three maps from the files `dds PREFIX` wrote; the specular loader goes by the file's DXGI format */
static PBR_IBLMaps load_maps(const char* prefix) {
    PBR_IBLMaps maps;
    memset(&maps, 0, sizeof maps);
    const char* names[3] = {"specular", "irradiance", "lut"};
    GPU_Texture** slots[3] = {&maps.tex_specular_env_map, &maps.irradiance_map, &maps.brdf_lut};
    for (int i = 0; i < 3; ++i) {
        char path[4096];
        uint8_t head[148];
        if (snprintf(path, sizeof path, "%s_%s.dds", prefix, names[i]) >= (int)sizeof path) { fprintf(stderr, "ddsin: path too long\n"); return maps; }
        FILE* f = fopen(path, "rb");
        const size_t got = f ? fread(head, 1, sizeof head, f) : 0;
        if (f) fclose(f);
        const uint32_t dxgi = got == sizeof head && head[84] == 'D' && head[85] == 'X' && head[86] == '1' && head[87] == '0'
                                  ? (uint32_t)head[128] | ((uint32_t)head[129] << 8) | ((uint32_t)head[130] << 16) | ((uint32_t)head[131] << 24) : 0;
        *slots[i] = i == 0 && dxgi == 95 ? PBR_MakeTextureFromBC6HDDSFile(path, GPU_Format_RGBA32F) : PBR_MakeTextureFromFloatDDSFile(path);
        if (!*slots[i]) { fprintf(stderr, "ddsin: cannot load %s\n", path); return maps; }
    }
    return maps;
}

int main(int argc, char** argv) {
    const char* sh9_path = NULL;
    const char* dds_prefix = NULL;
    const char* ddsin_prefix = NULL;
    const char* pano_prefix = NULL;
    int sh9shade = 0, dds_format = PBR_DDS_OUT_BC6H_UF16, ggx_samples = 0, ggx_lut = 0;
    if (argc >= 4 && strcmp(argv[argc - 2], "ggx") == 0) {
        ggx_samples = atoi(argv[argc - 1]); argc -= 2;
        if (ggx_samples < 1 || ggx_samples > 4096) { fprintf(stderr, "ggx: the sample count is 1 .. 4096\n"); return 2; }
    } else if (argc >= 4 && strcmp(argv[argc - 2], "ggxpair") == 0) {
        ggx_samples = atoi(argv[argc - 1]); ggx_lut = 1; argc -= 2;
        if (ggx_samples < 1 || ggx_samples > 4096) { fprintf(stderr, "ggxpair: the sample count is 1 .. 4096\n"); return 2; }
    }
    if (argc >= 4 && strcmp(argv[argc - 2], "pano") == 0) { pano_prefix = argv[argc - 1]; argc -= 2; }
    if (argc >= 3 && strcmp(argv[argc - 1], "sh9shade") == 0) { sh9shade = 1; argc -= 1; }
    if (argc >= 4 && strcmp(argv[argc - 2], "ddsin") == 0) { ddsin_prefix = argv[argc - 1]; argc -= 2; }
    if (argc >= 4 && strcmp(argv[argc - 2], "dds") == 0) { dds_prefix = argv[argc - 1]; argc -= 2; }
    else if (argc >= 4 && strcmp(argv[argc - 2], "dds2") == 0) { dds_prefix = argv[argc - 1]; dds_format = PBR_DDS_OUT_BC6H_UF16_2R; argc -= 2; }
    if (argc >= 4 && strcmp(argv[argc - 2], "sh9") == 0) { sh9_path = argv[argc - 1]; argc -= 2; }
    if (argc < 2) { fprintf(stderr, "usage: %s cube_strip.hdr [irr lut spec min_size [width height]]\n", argv[0]); return 2; }
    uint32_t irr = argc > 2 ? (uint32_t)atoi(argv[2]) : 32, lut = argc > 3 ? (uint32_t)atoi(argv[3]) : 256;
    uint32_t spec = argc > 4 ? (uint32_t)atoi(argv[4]) : 256, min_size = argc > 5 ? (uint32_t)atoi(argv[5]) : 16;
    uint32_t width = argc > 6 ? (uint32_t)atoi(argv[6]) : 320, height = argc > 7 ? (uint32_t)atoi(argv[7]) : 180;

    GPU_Init(NULL);                                                          /* main.cpp:35 */
    GPUX_EnableOpTiming(1);
    GPU_Texture* tex_env_cube = PBR_MakeTextureFromHDRIFile(argv[1]);        /* main.cpp:47 */
    if (!tex_env_cube) return 1;
    printf("env_size %u\nenv_mips %u\n", tex_env_cube->width, tex_env_cube->mip_level_count);
    if (sh9_path) {
        double coef[27], sum = 0.0;
        if (PBR_ProjectSH9(tex_env_cube, 0, coef) != 0 || PBR_WriteSH9File(sh9_path, coef) != 0) { fprintf(stderr, "sh9: cannot write %s\n", sh9_path); return 1; }
        for (int i = 0; i < 27; ++i) sum += coef[i];
        printf("sh9_sum %.17g\n", sum);
    }

    PBR_IBLMaps maps;
    if (ddsin_prefix) {
        maps = load_maps(ddsin_prefix);
        if (!maps.tex_specular_env_map || !maps.irradiance_map || !maps.brdf_lut) return 1;
        spec = maps.tex_specular_env_map->width;
    } else {
        PBR_MakeIBLMaps(&maps, irr, lut, spec);                              /* render.cpp:794-796 */
        PBR_GenIrradianceMap(tex_env_cube, maps.irradiance_map);             /* render.cpp:505-540 */
        if (ggx_samples) PBR_GenPrefilteredEnvMapGGX(tex_env_cube, maps.tex_specular_env_map, min_size, (uint32_t)ggx_samples);
        else PBR_GenPrefilteredEnvMap(tex_env_cube, maps.tex_specular_env_map, min_size);   /* render.cpp:542-589 */
        if (ggx_lut) PBR_GenBRDFIntegrationMapGGX(maps.brdf_lut, (uint32_t)ggx_samples, GPUX_BrdfLut_SmithSchlick);
        else PBR_GenBRDFIntegrationMap(maps.brdf_lut);                       /* render.cpp:591-619 */
    }

    printf("env_mip0_sum %.9e\n", checksum_texture_mip(tex_env_cube, 0, 1));
    printf("env_last_mip_sum %.9e\n", checksum_texture_mip(tex_env_cube, tex_env_cube->mip_level_count - 1, 1));
    printf("irradiance_sum %.9e\n", checksum_texture_mip(maps.irradiance_map, 0, 1));
    uint32_t size = spec;
    for (uint32_t m = 0; m < maps.tex_specular_env_map->mip_level_count && size >= min_size; ++m, size /= 2)
        printf("specular_mip%u_sum %.9e\n", m, checksum_texture_mip(maps.tex_specular_env_map, m, 1));
    printf("lut_bits_sum %.9e\n", checksum_texture_mip(maps.brdf_lut, 0, 0));
    if (dds_prefix) {
        uint32_t filtered = 0;                                               /* the levels the prefilter wrote */
        for (uint32_t sz = spec; filtered < maps.tex_specular_env_map->mip_level_count && sz >= min_size; sz /= 2) filtered++;
        struct { const char* name; GPU_Texture* tex; uint32_t levels; int format; } files[3] = {
            {"specular", maps.tex_specular_env_map, filtered, dds_format}, {"irradiance", maps.irradiance_map, 0, PBR_DDS_OUT_SAME},
            {"lut", maps.brdf_lut, 0, PBR_DDS_OUT_SAME}};
        for (int i = 0; i < 3; ++i) {
            char path[4096];
            size_t bytes = 0;
            void* data = PBR_EncodeTextureDDS(files[i].tex, 0, files[i].levels, files[i].format, &bytes);
            FILE* f = NULL;
            if (!data || snprintf(path, sizeof path, "%s_%s.dds", dds_prefix, files[i].name) >= (int)sizeof path || !(f = fopen(path, "wb")) ||
                fwrite(data, 1, bytes, f) != bytes || fclose(f) != 0) { fprintf(stderr, "dds: cannot write %s_%s.dds\n", dds_prefix, files[i].name); return 1; }
            free(data);
            printf("dds_bytes %s %zu\n", files[i].name, bytes);
        }
    }
    if (pano_prefix) {
        uint32_t sz = spec, levels = 0;                                      /* the levels the prefilter wrote (or the file held) */
        for (; levels < maps.tex_specular_env_map->mip_level_count && sz >= min_size; sz /= 2) levels++;
        for (uint32_t i = 0; i <= levels; ++i) {                             /* the irradiance map, then specular level i - 1 */
            GPU_Texture* cube = i == 0 ? maps.irradiance_map : maps.tex_specular_env_map;
            const uint32_t mip = i == 0 ? 0 : i - 1;
            uint32_t n = cube->width >> mip; if (n < 1) n = 1;
            char path[4096];
            const int len = i == 0 ? snprintf(path, sizeof path, "%s_irradiance.hdr", pano_prefix) : snprintf(path, sizeof path, "%s_specular_mip%u.hdr", pano_prefix, mip);
            if (len >= (int)sizeof path || PBR_WritePanoramaHDR(path, cube, mip, 0, 0) != 0) { fprintf(stderr, "pano: cannot write a panorama under %s\n", pano_prefix); return 1; }
            if (i == 0) printf("pano_extent irradiance %u %u\n", 4 * n, 2 * n); else printf("pano_extent specular_mip%u %u %u\n", mip, 4 * n, 2 * n);
        }
    }

    /* a flat synthetic G-buffer: lower half = rough gold floor facing +Z at NDC depth .998, upper half = sky */
    PBR_GBuffer gb;
    PBR_MakeGBuffer(&gb, width, height, GPU_Format_RGBA16F);                 /* render.cpp:680-693 */
    {
        size_t n = (size_t)width * height;
        uint8_t* rgba = (uint8_t*)malloc(n * 4);
        float* depth = (float*)malloc(n * 4);
        GPU_Graph* g = GPU_MakeGraph();
        struct { GPU_Texture* t; uint8_t v[4]; } planes[4] = {
            {gb.base_color, {255, 195, 86, 255}}, {gb.normal, {128, 128, 255, 255}}, {gb.orm, {255, 90, 255, 255}}, {gb.emissive, {0, 0, 0, 255}}};
        for (int p = 0; p < 4; ++p) {
            for (size_t i = 0; i < n; ++i) memcpy(rgba + 4 * i, planes[p].v, 4);
            GPU_Buffer* b = GPU_MakeBuffer((uint32_t)(n * 4), GPU_BufferFlag_CPU, rgba);
            GPU_OpCopyBufferToTexture(g, b, planes[p].t, 0, 1, 0);
            GPU_GraphSubmit(g); GPU_GraphWait(g);
            GPU_DestroyBuffer(b);
        }
        for (size_t i = 0; i < n; ++i) depth[i] = (i / width) >= height / 2 ? 0.998f : 1.0f;
        GPU_Buffer* b = GPU_MakeBuffer((uint32_t)(n * 4), GPU_BufferFlag_CPU, depth);
        GPU_OpCopyBufferToTexture(g, b, gb.depth, 0, 1, 0);
        GPU_GraphSubmit(g); GPU_GraphWait(g);
        GPU_DestroyBuffer(b); GPU_DestroyGraph(g);
        free(rgba); free(depth);
    }
    PBR_LightingPass* lp = PBR_MakeLightingPass(&gb, &maps, width, height);  /* render.cpp:716-723, 829-871 */
    PBR_Globals globals;
    float pos[3] = {0.f, 0.f, 5.f};                                          /* main.cpp:18 */
    PBR_FillGlobals(&globals, pos, NULL, 75.f, (float)width / (float)height, 0.02f, 10000.f, 56.5f, 97.f, 0);   /* main.cpp:21,85-88 */
    GPU_Graph* graph = GPU_MakeGraph();
    PBR_RecordLightingPass(lp, graph, &globals, 0, 0);                       /* render.cpp:1119-1127 */
    GPU_GraphSubmit(graph);
    GPU_GraphWait(graph);
    for (uint32_t i = 0; i < GPUX_GraphTimedOpCount(graph); ++i)
        printf("time_ms %s %.6f\n", GPUX_GraphTimedOpName(graph, i), GPUX_GraphTimedOpMs(graph, i));
    printf("lit_bits_sum %.9e\n", checksum_texture_mip(gb.lighting_result, 0, 0));

    /* ---- per-frame chain: lighting -> TAA -> bloom -> final, three frames (velocity buffers stay zero: a still camera) ---- */
    PBR_PostProcess* pp = PBR_MakePostProcess(&gb, width, height, GPU_Format_RGBA8UN);
    const int raster = argc > 9 && strcmp(argv[9], "raster") == 0;
    PBR_Material* material = NULL; PBR_Mesh* mesh = NULL; PBR_GeometryPass* gp = NULL;
    if (raster) {
        mesh = demo_mesh(&material);
        gp = PBR_MakeGeometryPass(&gb, pp, width, height);
        if (!mesh || !gp) return 1;
        printf("gbuffer_raster 1\n");
    }
    for (uint32_t frame = 0; frame < 3; ++frame) {
        PBR_FillGlobals(&globals, pos, NULL, 75.f, (float)width / (float)height, 0.02f, 10000.f, 56.5f, 97.f, frame);
        if (raster) {                                                        /* render.cpp:993, 1076-1115; a still camera */
            memcpy(globals.old_clip_space_from_world, globals.clip_space_from_world, sizeof globals.clip_space_from_world);
            PBR_RecordGeometryPass(gp, graph, mesh, NULL, &globals, NULL, NULL, frame);
        }
        PBR_RecordLightingPass(lp, graph, &globals, 0, 0);                   /* render.cpp:1119-1127 */
        PBR_RecordTaaResolve(pp, graph, frame);                              /* render.cpp:1131-1137 */
        PBR_RecordBloom(pp, graph, frame);                                   /* render.cpp:1139-1176 */
        PBR_RecordFinalPostProcessBloom(pp, graph, frame);                   /* render.cpp:1181-1187 */
        GPU_GraphSubmit(graph);
        GPU_GraphWait(graph);
    }
    for (uint32_t i = 0; i < GPUX_GraphTimedOpCount(graph); ++i)
        printf("time_ms %s %.6f\n", GPUX_GraphTimedOpName(graph, i), GPUX_GraphTimedOpMs(graph, i));
    printf("taa_bits_sum %.9e\n", checksum_texture_mip(PBR_PostTaaOutput(pp, 0), 0, 0));
    printf("bloom_bits_sum %.9e\n", checksum_texture_mip(PBR_PostBloomUpscale(pp), 0, 0));
    {
        GPU_Texture* bb = PBR_PostBackbuffer(pp);
        uint32_t bytes = (uint32_t)GPUX_TextureMipBytes(bb, 0);
        GPU_Buffer* buf = GPU_MakeBuffer(bytes, GPU_BufferFlag_CPU, NULL);
        GPU_Graph* g = GPU_MakeGraph();
        GPU_OpCopyTextureToBuffer(g, bb, buf);
        GPU_GraphSubmit(g); GPU_GraphWait(g);
        const uint8_t* px = (const uint8_t*)buf->data;
        double sum = 0.0;
        for (uint32_t i = 0; i < bytes; ++i) sum += (double)px[i];
        printf("frame_bytes_sum %.9e\n", sum);
        if (argc > 8) {                                                      /* binary PPM, rows top-down as rendered */
            FILE* f = fopen(argv[8], "wb");
            if (!f) { perror(argv[8]); return 1; }
            fprintf(f, "P6\n%u %u\n255\n", width, height);
            for (uint32_t i = 0; i < width * height; ++i) fwrite(px + 4 * i, 1, 3, f);
            fclose(f);
        }
        GPU_DestroyGraph(g); GPU_DestroyBuffer(buf);
    }

    /* ---- voxel light grid: clear, a ground slab of lit voxels, three sweeps (directions y, z, x); with `raster` the lit voxels are
     *      not a stand-in: the sun depth pass (render.cpp:995-1020) and the voxelise pass (:1039-1056) draw the built-in mesh ---- */
    if (raster) {
        PBR_Lightgrid* lg = PBR_MakeLightgrid(128);
        PBR_SunDepthPass* sun = PBR_MakeSunDepthPass(2048);
        PBR_VoxelizePass* vp = PBR_MakeVoxelizePass(lg, sun);
        if (!lg || !sun || !vp) return 1;
        GPU_Graph* g = GPU_MakeGraph();
        PBR_RecordLightgridClear(lg, g);                                     /* render.cpp:1028 */
        PBR_RecordSunDepthPass(sun, g, mesh, &globals);
        PBR_RecordVoxelizePass(vp, g, mesh, &globals);
        for (int k = 0; k < 3; ++k) PBR_RecordLightgridSweep(lg, g);         /* render.cpp:1061-1072 */
        GPU_GraphSubmit(g); GPU_GraphWait(g);
        for (uint32_t i = 0; i < GPUX_GraphTimedOpCount(g); ++i)
            printf("time_ms %s %.6f\n", GPUX_GraphTimedOpName(g, i), GPUX_GraphTimedOpMs(g, i));
        printf("lightgrid_voxelized 1\nlightgrid_bits_sum %.9e\n", checksum_texture_mip(PBR_LightgridTexture(lg), 0, 0));
        if (argc > 10 && strcmp(argv[10], "gridview") == 0) {               /* main.cpp:79: one more frame with visualize_lightgrid set (K16) */
            PBR_LightingPass* vlp = PBR_MakeLightingPassLive(&gb, &maps, width, height, NULL, PBR_LightgridTexture(lg), NULL);
            PBR_Globals vg = globals;
            vg.visualize_lightgrid = 1;
            PBR_RecordLightingPass(vlp, g, &vg, 0, 0);
            GPU_GraphSubmit(g); GPU_GraphWait(g);
            for (uint32_t i = 0; i < GPUX_GraphTimedOpCount(g); ++i)
                printf("time_ms %s %.6f\n", GPUX_GraphTimedOpName(g, i), GPUX_GraphTimedOpMs(g, i));
            printf("gridview_bits_sum %.9e\n", checksum_texture_mip(gb.lighting_result, 0, 0));
            PBR_DestroyLightingPass(vlp);
        }
        GPU_DestroyGraph(g);
        PBR_DestroyVoxelizePass(vp); PBR_DestroySunDepthPass(sun); PBR_DestroyLightgrid(lg);
    } else {
        PBR_Lightgrid* lg = PBR_MakeLightgrid(128);                          /* render.cpp:678 */
        GPU_Texture* grid = PBR_LightgridTexture(lg);
        uint32_t bytes = (uint32_t)GPUX_TextureMipBytes(grid, 0);
        uint16_t* vox = (uint16_t*)calloc(bytes, 1);
        for (uint32_t z = 0; z < 4; ++z)                                     /* RGBA16F: (0.5, 0.25, 0.125, 1) in the four lowest layers */
            for (uint32_t i = 0; i < 128 * 128; ++i) {
                uint16_t* v = vox + ((size_t)z * 128 * 128 + i) * 4;
                v[0] = 0x3800; v[1] = 0x3400; v[2] = 0x3000; v[3] = 0x3c00;
            }
        GPU_Buffer* up = GPU_MakeBuffer(bytes, GPU_BufferFlag_CPU, vox);
        GPU_Graph* g = GPU_MakeGraph();
        PBR_RecordLightgridClear(lg, g);                                     /* render.cpp:1028 */
        GPUX_OpCopyBufferToTextureMip(g, up, 0, grid, 0);
        for (int k = 0; k < 3; ++k) PBR_RecordLightgridSweep(lg, g);         /* render.cpp:1061-1072 */
        GPU_GraphSubmit(g); GPU_GraphWait(g);
        for (uint32_t i = 0; i < GPUX_GraphTimedOpCount(g); ++i)
            printf("time_ms %s %.6f\n", GPUX_GraphTimedOpName(g, i), GPUX_GraphTimedOpMs(g, i));
        printf("lightgrid_bits_sum %.9e\n", checksum_texture_mip(grid, 0, 0));
        GPU_DestroyGraph(g); GPU_DestroyBuffer(up); free(vox);
        PBR_DestroyLightgrid(lg);
    }
    if (raster) {
        printf("gbuffer_depth_sum %.9e\n", checksum_texture_mip(gb.depth, 0, 1));
        PBR_DestroyGeometryPass(gp); PBR_DestroyMesh(mesh); PBR_DestroyMaterial(material);
    }
    PBR_DestroyPostProcess(pp);
    if (sh9shade) {                                                          /* the coefficients never leave the device */
        GPU_Buffer* coef = GPU_MakeBuffer(27 * sizeof(double), GPU_BufferFlag_GPU, NULL);
        GPU_Graph* g = GPU_MakeGraph();
        if (!coef || !g) return 1;
        PBR_FillGlobals(&globals, pos, NULL, 75.f, (float)width / (float)height, 0.02f, 10000.f, 56.5f, 97.f, 0);
        GPUX_OpProjectSH9(g, tex_env_cube, 0, 0, 6, 0, tex_env_cube->width, coef, 0);
        PBR_LightingUseSH9(lp, coef, 0);
        PBR_RecordLightingPass(lp, g, &globals, 0, 0);
        GPU_GraphSubmit(g); GPU_GraphWait(g);
        PBR_LightingUseSH9(lp, NULL, 0);
        printf("frame_sh9_checksum %.9e\n", checksum_texture_mip(gb.lighting_result, 0, 0));
        GPU_DestroyGraph(g); GPU_DestroyBuffer(coef);
    }

    GPU_DestroyGraph(graph);
    PBR_DestroyLightingPass(lp);
    PBR_DestroyGBuffer(&gb);
    PBR_DestroyIBLMaps(&maps);
    GPU_DestroyTexture(tex_env_cube);
    GPU_WaitUntilIdle();
    GPU_Deinit();                                                            /* main.cpp:113 */
    printf("ok 1\n");
    return 0;
}
