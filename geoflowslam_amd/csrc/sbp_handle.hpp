// What triangulate.hip needs of a gfs_sbp handle (the struct itself is sbp.hip's): its device, stream, lock and capacities, and the
// slot that holds the triangulation workspace.
#pragma once
#include "gfs_common.hpp"

struct gfs_tri_workspace;  // triangulate.hip

struct gfs_sbp_core {
  int device, max_cur, max_batch;
  hipStream_t stream;
  std::mutex* mu;
  gfs_tri_workspace** tri;
};

gfs_sbp_core gfs_sbp_core_of(gfs_sbp* h);           // sbp.hip
void gfs_tri_workspace_free(gfs_tri_workspace* w);  // triangulate.hip; called by gfs_sbp_destroy
