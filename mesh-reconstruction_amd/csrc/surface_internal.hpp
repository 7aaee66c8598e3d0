// surface_internal.hpp -- the object behind mvs_surface (include/mvs.h), shared by csrc/poisson.hip and csrc/tsdf.hip (which fill it) and
// csrc/surface_criteria.cpp (which improves its facets in place).  Host-only: no HIP header (the stream is the runtime's opaque pointer).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct SurfaceGrid {
    int G;             // nodes per axis
    float ox, oy, oz;  // position of node (0, 0, 0)
    float h;           // node spacing
};

struct mvs_surface {
    SurfaceGrid grid{};
    float iso = 0.0f;
    float spacing = 0.0f;     // CGAL::compute_average_spacing(points, 6) of the samples
    int ratio_kept = 1;       // node spacing <= 0.75 x average spacing (0: the finest grid, 512^3, is coarser than that)
    int normal_scale_log2 = 0;  // the normals were multiplied by 2^this before the fixed-point splat (chi and the level scale with it)
    int support_cells = 0;    // cells are meshed within this many nodes of a node that collected sample weight (0: everywhere)
    std::vector<float> vertices;   // 4 per vertex
    std::vector<int32_t> faces;    // 3 per face
    std::vector<float> chi;        // G^3, kept when asked for (tests)
    std::vector<int64_t> splat;    // 4 G^3 (vx, vy, vz, weight), kept when asked for (tests)
};

struct ihipStream_t;  // hipStream_t

// csrc/poisson.hip: the surface-nets mesher of mvs_poisson_surface on a device field (G^3 floats in the node order (k G + j) G + i): one vertex
// per patch of every mixed cell, one quad per crossing grid edge, numbered in grid order, faces along +grad chi ("inside" = chi < iso).
// support (nullable, G^3 bytes): a cell is meshed only when the node at its low corner is non-zero.  Runs on `stream`, fills res->vertices and
// res->faces and synchronises the stream; nothing else of res is touched.  Returns MVS_OK, or an MVS_* code with `why` = who + ": " + reason.
int surface_nets_device(const SurfaceGrid &g, const float *chi, float iso, const unsigned char *support, ihipStream_t *stream, mvs_surface *res,
                        const char *who, std::string &why);
