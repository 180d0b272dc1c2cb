// wost_internal3.h -- host-side declarations shared by the translation units of the 3-D path (not part of the C-ABI): the
// uploaded mesh, the context behind wost3_handle.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/wost.h"
#include "wost_device3.h"
#include "wost_internal.h"
#include "wost_uniform.h"

namespace wost {

struct HostMesh3 {
    int32_t n_tris = 0, n_edges = 0, levels = 1, first_leaf = 1;
    bool emissive = false;
    std::vector<float> nodes, tri, colors, cones, slotEdges;
    float ext = 0.0f;                 // largest coordinate
    std::vector<int32_t> triOrig, triVerts, flatVerts;
    std::vector<float> obox;          // index-ordered run boxes (emissive meshes above the flat limit)
    int32_t obox_off[12] = {0}, obox_levels = 0;
    std::vector<DevTri> flat;
    std::vector<DevEdge3> edges;
};

struct DeviceMesh3 {
    DevMesh3 view{};
    HostMesh3 host;
    std::vector<void *> allocs;
};

// LDS bytes of the task pools (WavePool3) of a block of `waves` waves: per wave two pools of pool_cap tasks and the owners' words
inline size_t pool3_lds_bytes(int waves, int pool_cap) { return (size_t)waves * (2 * (size_t)pool_cap + kPool3OwnerWords) * sizeof(uint32_t); }

}  // namespace wost

// (the handle type of the C-ABI lives outside the namespace; its members are the namespace's.  device, settings, dst, mask, n_pixels,
// field, stream, the events and the carried states: HandleBase, wost_uniform.h)
struct wost3_context : wost::HandleBase {
    wost::DevProbe3 probe{};
    wost::DeviceMesh3 dm, nm;
    wost::DevSource3 src{};          // rgb owned by the context
    wost::Stats3Dev *stats = nullptr;
    uint32_t *cursor = nullptr;
    int wait_weight = 32, trav_burst = 3;   // a sweep over both constants: a leaf visit (four exact triangle distances) is dear, steps are served early
};

namespace wost {
// wost_build3.hip: the mesh of `d` built on the current device (records, Morton order, tree, cones) into s.view
int upload_mesh3(const wost3_mesh_desc &d, DeviceMesh3 &s);
// wost_vmm3.hip: dL/draw of the 3-D mixture loss for n training samples, all pointers on the device (rows of 41 floats)
void launch_vmm3_loss_gradients(hipStream_t stream, const float *raw, const float *dir, const float *li, const float *dir_pdf,
                                const unsigned char *on_neumann, const float *normal, int n, float loss_scale, float *dl_draw, float *likelihood);
}  // namespace wost
