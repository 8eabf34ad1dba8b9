/* pbr_mesh.h -- PBR_Mesh as the host sources that draw it see it (pbr_shadow.c owns it, pbr_geometry.c reads it). */
#ifndef PBR_MESH_H
#define PBR_MESH_H
#include "pbr_host.h"

struct PBR_Mesh {
    GPU_Buffer* vertex_buffer;
    GPU_Buffer* index_buffer;
    PBR_MeshPart* parts;
    PBR_Material** materials;      /* per part, NULL until PBR_MeshSetPartMaterial; not owned */
    uint32_t part_count;
};
#endif
