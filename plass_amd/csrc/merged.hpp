// plasship_merged (include/plasship_ext/linclust.h): what plasship_clusters_merge makes, for the modules that read it (merge_clusters.hip, repseqs.hip)
#pragma once
#include "common.hpp"

struct plasship_merged {
    size_t n = 0;                  // == DB size
    uint64_t nClusters = 0;
    uint64_t dbGen = 0;
    plasship::DevBuf d_pairs;      // uint64 [n]: representative id << 32 | member id, in the order of the merged DB
};
