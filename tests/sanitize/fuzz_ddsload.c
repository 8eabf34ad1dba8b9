// sanitizer harness for the way from a .dds file to a texture (host/pbr_dds.c + host/pbr_ddsin.c, run on CPU only) over a recording
// fake of the GPU entry points those two files call: textures are described as the backend describes them, buffers are heap memory of
// exactly the requested size, ops are recorded and carried out at GPU_GraphSubmit as copies of the staged bytes into per-level heap
// blocks.  Files are exact-size heap copies, so ASan sees every byte a loader or the fake reads.
//   1. files laid out by PBR_BuildDDSHeader around random payloads, extents 1 .. 40, every level count, 2-D and cube, through the loader
//      of their format: whether the loader takes the file is this harness's own restatement of the loader's rule; what reaches every
//      level must be the file's bytes of that level, layer after layer, by one op per level, levels ascending, one submit.
//   2. the mutations of fuzz_dds.c / fuzz_ddsex.c through all three loaders: NULL, or levels that are the bytes PBR_ParseDDSEx describes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "pbr_host.h"

#define FAIL(code, ...) do { fprintf(stderr, "fuzz_ddsload: " __VA_ARGS__); fprintf(stderr, "\n"); exit(code); } while (0)

/* ---- the fake ---- */
typedef struct FakeTexture { GPU_Texture base; uint8_t* level[PBR_DDS_MAX_LEVELS]; uint64_t level_bytes[PBR_DDS_MAX_LEVELS]; } FakeTexture;
typedef struct Op { int decode; GPU_Buffer* buf; uint32_t offset; GPU_Texture* tex; uint32_t mip; } Op;
struct GPU_Graph { Op ops[PBR_DDS_MAX_LEVELS]; uint32_t op_count; int submits, waits; };
static struct { Op ops[PBR_DDS_MAX_LEVELS]; uint32_t op_count; int submits, waits, graphs, buffers; } seen;   /* of the last loader call */
static int live_textures, live_buffers, live_graphs;

static uint32_t dim(uint32_t d, uint32_t m) { return d >> m ? d >> m : 1; }
static uint64_t mip_bytes(const GPU_Texture* t, uint32_t m) {                  /* all layers, as GPUX_TextureMipBytes counts */
    const GPU_Format f = t->format;
    const int bc = f == GPU_Format_BC1_RGBA_UN || f == GPU_Format_BC3_RGBA_UN || f == GPU_Format_BC5_UN;
    const uint64_t unit = f == GPU_Format_BC1_RGBA_UN ? 8 : (bc || f == GPU_Format_RGBA32F) ? 16 : f == GPU_Format_RGBA16F ? 8 : 4;   /* RGBA8UN, RG16F: 4 */
    const uint64_t w = dim(t->width, m), h = dim(t->height, m);
    return (bc ? ((w + 3) / 4) * ((h + 3) / 4) : w * h) * unit * t->layer_count;
}
static void store_level(FakeTexture* t, uint32_t m, const void* src, uint64_t n) {
    free(t->level[m]);
    t->level[m] = (uint8_t*)malloc((size_t)n);
    memcpy(t->level[m], src, (size_t)n);
    t->level_bytes[m] = n;
}

GPU_Texture* GPU_MakeTexture(GPU_Format format, uint32_t width, uint32_t height, uint32_t depth, GPU_TextureFlags flags, const void* data) {
    if (!width || !height || depth != 1) FAIL(20, "GPU_MakeTexture: extent %u x %u x %u", width, height, depth);
    if (format != GPU_Format_RGBA8UN && format != GPU_Format_BC1_RGBA_UN && format != GPU_Format_BC3_RGBA_UN && format != GPU_Format_BC5_UN &&
        format != GPU_Format_RGBA32F && format != GPU_Format_RGBA16F && format != GPU_Format_RG16F) FAIL(20, "GPU_MakeTexture: format %d", (int)format);
    if (data && (flags & GPU_TextureFlag_HasMipmaps)) FAIL(20, "GPU_MakeTexture: data with a chain to generate");
    FakeTexture* t = (FakeTexture*)calloc(1, sizeof *t);
    t->base.width = width; t->base.height = height; t->base.depth = 1; t->base.format = format; t->base.flags = flags;
    t->base.layer_count = (flags & GPU_TextureFlag_Cubemap) ? 6 : 1;
    t->base.mip_level_count = 1;
    if (flags & GPU_TextureFlag_HasMipmaps)
        for (uint32_t s = width < height ? width : height; s > 1; s /= 2) t->base.mip_level_count++;
    if (data) store_level(t, 0, data, mip_bytes(&t->base, 0));
    live_textures++;
    return &t->base;
}
void GPU_DestroyTexture(GPU_Texture* texture) {
    if (!texture) return;
    FakeTexture* t = (FakeTexture*)texture;
    for (uint32_t m = 0; m < PBR_DDS_MAX_LEVELS; ++m) free(t->level[m]);
    free(t);
    live_textures--;
}
GPU_Buffer* GPU_MakeBuffer(uint32_t size, GPU_BufferFlags flags, const void* data) {
    if (size == 0 || flags != GPU_BufferFlag_CPU) FAIL(21, "GPU_MakeBuffer: size %u flags %d", size, flags);
    GPU_Buffer* b = (GPU_Buffer*)calloc(1, sizeof *b);
    b->flags = flags; b->size = size; b->data = malloc(size);
    if (data) memcpy(b->data, data, size);
    live_buffers++; seen.buffers++;
    return b;
}
void GPU_DestroyBuffer(GPU_Buffer* b) { if (b) { free(b->data); free(b); live_buffers--; } }
GPU_Graph* GPU_MakeGraph(void) { live_graphs++; seen.graphs++; return (GPU_Graph*)calloc(1, sizeof(GPU_Graph)); }
static void record(GPU_Graph* g, int decode, GPU_Buffer* buf, uint32_t offset, GPU_Texture* tex, uint32_t mip) {
    if (!g || !buf || !tex || g->submits || g->op_count == PBR_DDS_MAX_LEVELS) FAIL(22, "an op with a NULL argument, after the submit, or too many");
    g->ops[g->op_count++] = (Op){decode, buf, offset, tex, mip};
}
void GPUX_OpCopyBufferToTextureMip(GPU_Graph* g, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* dst, uint32_t mip) { record(g, 0, src, src_offset, dst, mip); }
void GPUX_OpDecodeBC6H(GPU_Graph* g, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* dst, uint32_t mip) { record(g, 1, src, src_offset, dst, mip); }
uint64_t GPUX_BC6HMipBytes(const GPU_Texture* t, uint32_t m) {
    if (!t || m >= t->mip_level_count || t->depth != 1 || (t->format != GPU_Format_RGBA32F && t->format != GPU_Format_RGBA16F)) return 0;
    return (uint64_t)((dim(t->width, m) + 3) / 4) * ((dim(t->height, m) + 3) / 4) * 16 * t->layer_count;
}
void GPU_GraphSubmit(GPU_Graph* g) {                                          /* the ops run here: the staging buffer is read now */
    if (g->submits++) FAIL(23, "a graph submitted twice");
    for (uint32_t k = 0; k < g->op_count; ++k) {
        const Op* o = &g->ops[k];
        const uint64_t n = o->decode ? GPUX_BC6HMipBytes(o->tex, o->mip) : mip_bytes(o->tex, o->mip);
        if (o->mip >= o->tex->mip_level_count || n == 0 || (o->decode && o->offset % 16) || (uint64_t)o->offset + n > o->buf->size)
            FAIL(23, "op %u: level %u, %llu bytes at %u of a buffer of %u", k, o->mip, (unsigned long long)n, o->offset, o->buf->size);
        store_level((FakeTexture*)o->tex, o->mip, (const uint8_t*)o->buf->data + o->offset, n);
    }
    memcpy(seen.ops, g->ops, sizeof seen.ops); seen.op_count = g->op_count;
    seen.submits++;
}
void GPU_GraphWait(GPU_Graph* g) { if (g->submits != 1 || g->waits++) FAIL(23, "a wait without its submit"); seen.waits++; }
void GPU_DestroyGraph(GPU_Graph* g) { if (g) { free(g); live_graphs--; } }

/* ---- the harness ---- */
static uint32_t rs = 2463534242u;
static uint32_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 17; rs ^= rs << 5; return rs; }
static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

static const uint32_t DXGI[8] = {71, 77, 83, 28, 2, 10, 34, 95};
static long loaded, refused;

/* loader: 0 material without PBR_DDS_FILE_MIPS, 1 material with it, 2 float, 3 BC6H (into RGBA16F or RGBA32F by the low bit of `pick`).
 * The texture (or NULL) of an exact-size heap copy of the file, after the checks that hold for every call: nothing but the texture
 * outlives it; its ops are one per level in ascending order, of the loader's kind, in one graph submitted and waited for once. */
static GPU_Texture* load(int loader, const uint8_t* file, size_t n, uint32_t pick, uint8_t** exact_out) {
    uint8_t* exact = (uint8_t*)malloc(n ? n : 1);
    memcpy(exact, file, n);
    memset(&seen, 0, sizeof seen);
    GPU_Texture* t = loader <= 1 ? PBR_MakeTextureFromDDSMemory(exact, n, loader ? PBR_DDS_FILE_MIPS : 0)
                   : loader == 2 ? PBR_MakeTextureFromFloatDDSMemory(exact, n)
                                 : PBR_MakeTextureFromBC6HDDSMemory(exact, n, (pick & 1) ? GPU_Format_RGBA16F : GPU_Format_RGBA32F);
    if (live_textures != (t ? 1 : 0) || live_buffers || live_graphs) FAIL(30, "loader %d left %d textures, %d buffers, %d graphs", loader, live_textures, live_buffers, live_graphs);
    if (!t && seen.submits) FAIL(30, "loader %d submitted and then refused", loader);
    if (t && seen.graphs && (seen.graphs != 1 || seen.buffers != 1 || seen.submits != 1 || seen.waits != 1 || seen.op_count == 0))
        FAIL(30, "loader %d: %d graphs, %d buffers, %d submits, %d waits, %u ops", loader, seen.graphs, seen.buffers, seen.submits, seen.waits, seen.op_count);
    for (uint32_t k = 0; t && k < seen.op_count; ++k)
        if (seen.ops[k].mip != k || seen.ops[k].decode != (loader == 3) || seen.ops[k].tex != t) FAIL(30, "loader %d: op %u is of level %u", loader, k, seen.ops[k].mip);
    if (t) loaded++; else refused++;
    *exact_out = exact;
    return t;
}
/* levels [0, n) of t hold the file's bytes of that level, layer after layer; the others were never written */
static void verify(const GPU_Texture* tex, const uint8_t* exact, const PBR_DDSInfoEx* lay, uint32_t n, const char* what) {
    const FakeTexture* t = (const FakeTexture*)tex;
    for (uint32_t m = 0; m < PBR_DDS_MAX_LEVELS; ++m) {
        if (m >= n) { if (t->level[m]) FAIL(31, "%s: level %u was written", what, m); continue; }
        if (!t->level[m] || t->level_bytes[m] != lay->level_size[m] * lay->layers) FAIL(31, "%s: level %u holds %llu bytes", what, m, (unsigned long long)t->level_bytes[m]);
        for (uint32_t l = 0; l < lay->layers; ++l)
            if (memcmp(t->level[m] + l * lay->level_size[m], exact + lay->level_offset[l][m], (size_t)lay->level_size[m])) FAIL(31, "%s: level %u layer %u is not the file's", what, m, l);
    }
}
static uint32_t chain(uint32_t w, uint32_t h, int smaller) {
    uint32_t n = 1;
    for (uint32_t s = (w < h) == (smaller != 0) ? w : h; s > 1; s >>= 1) n++;
    return n;
}
/* how many levels `loader` uploads of a well-formed file, by the rules of include/pbr_host.h; 0: it refuses the file */
static uint32_t levels_taken(int loader, uint32_t dxgi, uint32_t w, uint32_t h, uint32_t layers, uint32_t levels) {
    const int material = dxgi == 71 || dxgi == 77 || dxgi == 83 || dxgi == 28, flt = dxgi == 2 || dxgi == 10 || dxgi == 34;
    const uint32_t tex_levels = chain(w, h, 1);
    if (loader <= 1) {
        if (!material || layers != 1) return 0;
        if (loader == 0 || levels == 1) return 1;
        return levels >= tex_levels ? tex_levels : 0;
    }
    if (loader == 2) return flt && (levels == 1 || levels == tex_levels) ? levels : 0;
    return dxgi == 95 && (levels == 1 || levels <= tex_levels) ? levels : 0;
}

static uint8_t file[148 + 6 * 70000];

static void well_formed(int loader, uint32_t dxgi, uint32_t w, uint32_t h, uint32_t layers, uint32_t levels) {
    PBR_DDSInfoEx lay;
    const uint64_t n = PBR_BuildDDSHeader(dxgi, w, h, layers, levels, file, &lay);
    if (n == 0 || n > sizeof file) FAIL(40, "no file for format %u, %u x %u, %u layers, %u levels", dxgi, w, h, layers, levels);
    for (uint64_t k = 148; k < n; ++k) file[k] = (uint8_t)rnd();
    uint8_t* exact;
    char what[96];
    snprintf(what, sizeof what, "loader %d, format %u, %u x %u, %u layers, %u levels", loader, dxgi, w, h, layers, levels);
    GPU_Texture* t = load(loader, file, (size_t)n, w + h, &exact);
    const uint32_t want = levels_taken(loader, dxgi, w, h, layers, levels);
    if ((t != NULL) != (want != 0)) FAIL(41, "%s: %s", what, t ? "taken" : "refused");
    if (t) {
        const int direct = loader == 0 || (loader == 1 && levels == 1);       /* GPU_MakeTexture takes level 0 itself: no op */
        const uint32_t tex_levels = (loader == 0 || levels == 1) ? 1 : chain(w, h, 1);
        if (t->width != w || t->height != h || t->layer_count != layers || t->mip_level_count != tex_levels) FAIL(41, "%s: a %u x %u texture of %u layers, %u levels", what, t->width, t->height, t->layer_count, t->mip_level_count);
        if (seen.op_count != (direct ? 0 : want)) FAIL(41, "%s: %u ops", what, seen.op_count);
        verify(t, exact, &lay, want, what);
        GPU_DestroyTexture(t);
    }
    free(exact);
}

int main(void) {
    for (uint32_t w = 1; w <= 40; ++w) {
        const uint32_t heights[3] = {w, 1 + (w * 7) % 40, 1 + (w + 12) % 40};   /* square, and two others: 40 x 1, 3 x 22, 12 x 5, ... */
        for (int k = 0; k < 3; ++k) {
            const uint32_t h = heights[k];
            for (uint32_t levels = 1; levels <= chain(w, h, 0); ++levels)
                for (int f = 0; f < 8; ++f) {
                    if (f < 4) { well_formed(0, DXGI[f], w, h, 1, levels); well_formed(1, DXGI[f], w, h, 1, levels); }
                    else {
                        well_formed(f == 7 ? 3 : 2, DXGI[f], w, h, 1, levels);
                        if (k == 0) well_formed(f == 7 ? 3 : 2, DXGI[f], w, w, 6, levels);
                    }
                }
        }
    }
    const long well_loaded = loaded, well_refused = refused;
    {   /* each loader refuses the others' formats, and the material loader cubes */
        well_formed(0, 2, 16, 16, 1, 1); well_formed(1, 95, 16, 16, 1, 5); well_formed(2, 71, 16, 16, 1, 1); well_formed(2, 95, 16, 16, 6, 5);
        well_formed(3, 10, 16, 16, 6, 5); well_formed(3, 77, 16, 16, 1, 1); well_formed(1, 28, 16, 16, 6, 1);
    }
    for (int iter = 0; iter < 4000; ++iter) {
        const uint32_t layers = (rnd() & 1) ? 6 : 1, w = 1 + rnd() % 96, h = layers == 6 ? w : 1 + rnd() % 96;
        const uint32_t levels = 1 + rnd() % chain(w, h, 0);
        const uint64_t total = PBR_BuildDDSHeader(DXGI[rnd() % 8], w, h, layers, levels, file, NULL);
        if (total == 0) FAIL(42, "no header for %u x %u, %u layers, %u levels", w, h, layers, levels);
        size_t n = total > sizeof file ? sizeof file : (size_t)total;
        for (size_t k = 148; k < n; ++k) file[k] = (uint8_t)rnd();
        const size_t hs = 148;
        switch (rnd() % 7) {
        case 0: n = rnd() % (n + 1); break;                                                          /* truncate */
        case 1: for (int k = 0; k < 1 + (int)(rnd() % 6); ++k) file[rnd() % hs] ^= (uint8_t)(1u << (rnd() % 8)); break;   /* bit flips in the header */
        case 2: wr32(file + 12 + 4 * (rnd() & 1), (rnd() & 1) ? 0xFFFFFFFFu - rnd() % 8 : (1u << (14 + rnd() % 18)) + rnd() % 3); break;   /* huge extents */
        case 3: wr32(file + 28, (rnd() & 1) ? 10 + rnd() % 100 : 0x80000000u + rnd()); break;        /* lying level count */
        case 4: wr32(file + 12, rnd()); wr32(file + 16, rnd()); wr32(file + 28, rnd()); break;
        case 5: break;                                                                               /* as written (or cut at the buffer's size) */
        default: for (size_t k = rnd() % hs; k < hs; ++k) file[k] = (uint8_t)rnd(); break;           /* garbage tail of the header */
        }
        for (int loader = 0; loader < 4; ++loader) {
            uint8_t* exact;
            GPU_Texture* t = load(loader, file, n, rnd(), &exact);
            if (t) {
                PBR_DDSInfoEx info;
                if (PBR_ParseDDSEx(exact, n, &info) != 0) FAIL(43, "loader %d took a file the parser refuses", loader);
                const uint32_t taken = seen.op_count ? seen.op_count : 1;
                if (taken > info.level_count || info.layers != t->layer_count) FAIL(43, "loader %d took %u levels of %u", loader, taken, info.level_count);
                verify(t, exact, &info, taken, "mutated file");
                GPU_DestroyTexture(t);
            }
            free(exact);
        }
    }
    if (!well_loaded || !well_refused || loaded == well_loaded || refused == well_refused) FAIL(44, "an outcome was never reached");
    printf("ok: %ld files loaded, %ld refused (as laid out by the writer: %ld, %ld)\n", loaded, refused, well_loaded, well_refused);
    return 0;
}
