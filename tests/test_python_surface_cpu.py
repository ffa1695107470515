"""CPU: the public Python surface of the scene handle and of the query front ends — every public method of _binding.Scene and every public function of
spira_hip.query with its parameters, their order and their defaults, as written down here.  The private helpers behind them may be shared and reshaped;
a caller's code must not notice.  No library and no device needed."""
import inspect

from spira_hip import _binding, query

SCENE = {
    "cast": "(self, rays8, want_normal=False, inplace=False, want_prim=True, want_t=True)",
    "cast_device": "(self, d_rays_ptr, n_rays, d_prim_ptr, d_t_ptr, d_normal_ptr, stream_ptr, inplace=False)",
    "cast_hits": "(self, rays8, max_hits, inplace=False, count_all=False, want_prim=True, want_t=True, want_count=True)",
    "cast_hits_device": "(self, d_rays_ptr, n_rays, max_hits, d_prim_ptr, d_t_ptr, d_count_ptr, stream_ptr, inplace=False, count_all=False)",
    "closest_point": "(self, points4, inplace=False, want_prim=True, want_dist=True, want_point=True, want_trips=False)",
    "closest_point_device": "(self, d_points_ptr, n_points, d_prim_ptr, d_dist_ptr, d_point_ptr, stream_ptr, inplace=False, d_trips_ptr=0)",
    "destroy": "(self)",
    "gather": "(self, points6, spp, max_depth, seed=0, sample0=0, key0=0, flags=0, sums=None, want_valid=False)",
    "gather_device": "(self, d_points_ptr, n_points, spp, max_depth, d_sums_ptr, seed=0, sample0=0, key0=0, flags=0, d_valid_ptr=0, stream_ptr=0)",
    "gather_visible": "(self, points6, spp, t_min=0.001, t_max=inf, seed=0, sample0=0, key0=0, counts=None, want_valid=False, inplace=False)",
    "gather_visible_device": "(self, d_points_ptr, n_points, spp, d_counts_ptr, t_min=0.001, t_max=inf, seed=0, sample0=0, key0=0, d_valid_ptr=0, stream_ptr=0, inplace=False)",
    "nearest_k": "(self, points4, max_near, inplace=False, count_all=False, want_prim=True, want_dist=True, want_point=True, want_count=True, want_trips=False)",
    "nearest_k_device": "(self, d_points_ptr, n_points, max_near, d_prim_ptr, d_dist_ptr, d_point_ptr, d_count_ptr, stream_ptr, inplace=False, count_all=False, d_trips_ptr=0)",
    "occluded": "(self, rays8, inplace=False)",
    "occluded_device": "(self, d_rays_ptr, n_rays, d_hit_ptr, stream_ptr, inplace=False)",
    "overlap_any": "(self, boxes10, inplace=False)",
    "overlap_any_device": "(self, d_boxes_ptr, n, d_hit_ptr, stream_ptr, inplace=False)",
    "overlap_box": "(self, boxes10, max_list, inplace=False, want_prim=True, want_count=True, want_trips=False)",
    "overlap_box_device": "(self, d_boxes_ptr, n, max_list, d_prim_ptr, d_count_ptr, stream_ptr, inplace=False, d_trips_ptr=0)",
    "params": "(self, width, height, spp, max_depth, **kw)",
    "radiance": "(self, rays6, spp, max_depth, seed=0, sample0=0, key0=0, flags=0, sums=None, want_valid=False)",
    "radiance_device": "(self, d_rays_ptr, n_rays, spp, max_depth, d_sums_ptr, seed=0, sample0=0, key0=0, flags=0, d_valid_ptr=0, stream_ptr=0)",
    "rebuild": "(self, triangles10)",
    "rebuild_device": "(self, triangles, stream=None)",
    "render": "(self, camera12, params, want_hdr=True, want_img=False)",
    "render_adaptive": "(self, camera12, params, adaptive, want_hdr=True, want_img=False, want_spp=True, want_q=True)",
    "render_adaptive_device": "(self, camera12, params, adaptive, d_hdr_ptr, d_img_ptr, d_spp_ptr, d_q_ptr, stream_ptr)",
    "render_device": "(self, camera12, params, d_hdr_ptr, d_img_ptr, stream_ptr)",
    "render_features": "(self, camera12, params, want_albedo=True, want_normal=True, want_depth=True)",
    "render_features_device": "(self, camera12, params, d_albedo_ptr, d_normal_ptr, d_depth_ptr, stream_ptr)",
    "render_multi": "(self, camera12, params, n_devices=None, want_hdr=True, want_img=False)",
    "signed_distance": "(self, points4, inplace=False, want_point=True, want_crossings=False, want_trips=False, want_prim=True, want_dist=True, want_inside=True)",
    "signed_distance_device": "(self, d_points_ptr, n_points, d_prim_ptr, d_dist_ptr, d_point_ptr, d_inside_ptr, stream_ptr, inplace=False, d_crossings_ptr=0, d_trips_ptr=0)",
    "sweep": "(self, rays8, radii, inplace=False, want_prim=True, want_t=True, want_point=True, want_normal=True, want_trips=False)",
    "sweep_blocked": "(self, rays8, radii, inplace=False)",
    "sweep_blocked_device": "(self, d_rays_ptr, d_radii_ptr, n, d_hit_ptr, stream_ptr, inplace=False)",
    "sweep_device": "(self, d_rays_ptr, d_radii_ptr, n, d_prim_ptr, d_t_ptr, d_point_ptr, d_normal_ptr, stream_ptr, inplace=False, d_trips_ptr=0)",
    "update": "(self, spheres5=None, materials8=None, triangles10=None)",
    "update_device": "(self, triangles, stream=None)",
}
QUERY = {
    "box_axes": "(quat)",
    "boxes_from_bounds": "(lo, hi)",
    "cast_all": "(scene, rays, max_hits, count_all=False, inplace=False, want_prim=True, want_t=True, stream=None)",
    "cast_rays": "(scene, rays, want_normal=False, occlusion=False, inplace=False, stream=None)",
    "closest_point_sphere": "(c, radius, p)",
    "closest_point_triangle": "(v0, e1, e2, p)",
    "closest_points": "(scene, points, inplace=False, want_point=True, want_trips=False, stream=None)",
    "count_hits": "(scene, rays, inplace=False, stream=None)",
    "count_within": "(scene, points, radius=None, inplace=False, stream=None)",
    "distance_field": "(scene, lo, hi, dims, band=None, stream=None)",
    "inside_mesh": "(scene, points, max_hits=16)",
    "inside_points": "(scene, points, stream=None)",
    "inside_spheres": "(spheres5, points, dtype)",
    "k_nearest": "(scene, points, k, count_all=False, inplace=False, want_prim=True, want_dist=True, want_point=True, want_trips=False, stream=None)",
    "normalize_rays": "(rays8, dtype, frame=None)",
    "overlap_box_sphere": "(centre, radius, c, h, A)",
    "overlap_box_triangle": "(v0, e1, e2, c, h, A)",
    "overlap_boxes": "(scene, boxes, max_list, any=False, inplace=False, want_trips=False, stream=None)",
    "prepare_boxes": "(boxes10, dtype, frame=None)",
    "prepare_points": "(points4, dtype, frame=None)",
    "prepare_sweeps": "(rays8, radii, dtype, frame=None)",
    "signed_distance": "(scene, points, inplace=False, want_point=True, want_crossings=False, want_trips=False, stream=None)",
    "signed_distance_rules": "(valid, prim, dist, point, in_sphere, counts, has_triangles)",
    "sweep_segments": "(scene, a, b, radius)",
    "sweep_sphere_sphere": "(c, radius, o, d, r, t_min, t_max)",
    "sweep_sphere_triangle": "(v0, e1, e2, o, d, r, t_min, t_max)",
    "sweep_spheres": "(scene, rays, radii, blocked=False, inplace=False, want_point=True, want_normal=True, want_trips=False, stream=None)",
    "voxel_boxes": "(lo, hi, dims, dtype)",
    "voxelize": "(scene, lo, hi, dims, stream=None)",
}


def test_scene_methods_keep_their_signatures():
    have = {name: str(inspect.signature(f)) for name, f in vars(_binding.Scene).items() if not name.startswith("_") and callable(f)}
    assert have == SCENE


def test_query_functions_keep_their_signatures():
    have = {name: str(inspect.signature(f)) for name, f in vars(query).items()
            if not name.startswith("_") and inspect.isfunction(f) and f.__module__ == query.__name__}
    assert have == QUERY
