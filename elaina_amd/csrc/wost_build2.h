// wost_build2.h -- the 2-D segment tree built on the device and the upload of a mesh into a handle (wost_build2.hip).  Not part
// of the C-ABI.
#pragma once

#include <cstddef>
#include <vector>

#include "../../include/wost.h"
#include "lbvh.h"
#include "wost_device.h"

namespace wost {

struct DeviceMeshStorage;      // the uploaded mesh of a handle (wost_internal2.h)

// the uploaded tree of one boundary mesh: `view` points into ONE device allocation (`alloc`, `bytes`) that the caller owns
struct DeviceTree2 {
    DevMesh view;
    void *alloc = nullptr;
    size_t bytes = 0;
};

// Problem<2>::build_bvh on the current device: segment records, Morton order, the refined leaf assignment, oriented child boxes,
// normal cones and the scan copies of `d`, the same bits as lbvh_build.cpp's build_tree + the uploads of upload_mesh
// (view.obox / lens / sampBox -- the run boxes of an emissive boundary on the tree -- are left to the caller).
// WOST_OK, or an error recorded with set_error.
int build_tree_device(const wost_mesh_desc &d, DeviceTree2 &out);

// (hidden: the dynamic symbol table of the library stays the C-ABI and what it held before; nothing here joins it)
#pragma GCC visibility push(hidden)
// The mesh of `d` on the current device, into s.view: built on the device for every mesh worth the launches, by the host builder
// for the small ones, behind WOST_HOST_BUILD=1 and for the tree-quality knobs.
int upload_mesh(const wost_mesh_desc &d, DeviceMeshStorage &s);
// ... by the host builder (lbvh_build.cpp), uploaded array by array: what wost_mesh_build_check compares the device build with
int upload_mesh_host(const wost_mesh_desc &d, DeviceMeshStorage &s);
// the run boxes over consecutive ORIGINAL indices and the sampler's compact copies (an emissive boundary on the tree only):
// a function of the flat records alone
int upload_run_boxes(const std::vector<FlatSeg> &flat_recs, DeviceMeshStorage &s);
#pragma GCC visibility pop

}  // namespace wost
