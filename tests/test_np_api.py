"""The non-physical path tracer's scene entry points (rt_scene_add_np_sphere / rt_scene_add_np_scene), host side."""
import pytest

from _rt import rt

OK = dict(center=(0.0, 0.0, -1.0), radius=0.5, kind=rt.NP_DIELECTRIC, refractive_index=1.5)


@pytest.mark.parametrize("bad", [dict(radius=0.0), dict(center=(0.0, float("nan"), -1.0)), dict(refractive_index=0.0),
                                 dict(refractive_index=-1.5), dict(kind=3), dict(radius=float("inf")),
                                 dict(albedo=(0.5, float("inf"), 0.5)), dict(fuzziness=float("nan"))])
def test_bad_sphere_is_invalid(bad):
    s = rt.Scene()
    with pytest.raises(rt.RtError) as e:
        s.add_np_sphere(**{**OK, **bad})
    assert e.value.status == rt.RT_ERR_INVALID
    assert s.add_np_sphere(**{**OK, "radius": -0.05}) == 0 and s.np_count() == 1   # a negative radius is a hollow


def test_np_spheres_do_not_mix():
    np_scene = rt.Scene()
    np_scene.add_np_sphere(**OK)
    for call in (lambda: rt.Scene.cornell().add_np_sphere(**OK),
                 lambda: np_scene.add_mesh(list(range(9)), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0))):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.status == rt.RT_ERR_INVALID


def test_np_scene_builds_six_spheres():
    s, i = rt.Scene.np_scene(), rt.Scene.np_scene().info()
    assert s.np_count() == 6 and (i.n_tris, i.n_nodes, i.n_meshes, i.n_spheres, i.light_mesh, i.device_bytes) == (0, 0, 0, 0, 0, 0)
