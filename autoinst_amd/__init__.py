"""autoinst_amd -- MI355X-native NCuts hot path of artonson/autoinst.

Affinity build + recursive normalized cut as hand-written HIP kernels (gfx950) behind the
reference's own Python call surface.  See DESIGN.md and include/autoinst_hip.h.
"""
from .config import CONFIG, CONFIG_SPATIAL, CONFIG_TARL_SPATIAL, CONFIG_TARL_SPATIAL_DINO, PROXIMITY_THRESHOLD, SPLIT_LIM  # noqa: F401


def __getattr__(name):
    # compute entry points load the HIP library on first use and raise if it is missing
    if name in ("normalized_cut", "ncuts", "get_affinity_matrix", "build_affinity", "build_affinity_batch", "ncuts_chunk", "ncuts_labels",
                "ncuts_labels_batch", "Context", "DeviceGraph", "default_context", "last_stats", "fiedler", "sweep", "lsym_apply", "bench_spmv", "eigs_smallest",
                "CutTree", "ncuts_tree", "ncuts_tree_batch", "relabel", "normalized_cut_sweep"):
        from . import ncuts_api as _n
        return getattr(_n, name)
    if name in ("Metrics", "score", "label_pairs", "merge_chunks_unite_instances2", "merge_associate", "unique_points", "merge_map",
                "label_tables", "remove_semantics", "score_sweep", "label_scores"):
        from . import labels_api as _l
        return getattr(_l, name)
    if name in ("box_select", "statistical_inlier_indices", "voxel_down_sample", "chunks_from_pointcloud",
                "chunk_and_downsample_point_clouds", "voxel_down_sample_nearest", "downsample_map"):
        from . import prep_api as _p
        return getattr(_p, name)
    if name in ("camera_features", "image_based_features_per_patch", "hidden_point_removal", "masks_to_image",
                "hidden_point_removal_device", "visible_sets"):
        from . import camera_api as _c
        return getattr(_c, name)
    if name in ("dbscan", "clusters_dbscan", "clusterize_pcd", "keep_largest_labels"):
        from . import cluster_api as _d
        return getattr(_d, name)
    raise AttributeError(name)
