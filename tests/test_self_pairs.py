"""(not gpu) vgt_hip_self_collision_pairs, the host-only pair generator (no context, no device), against
tests/self_ref.py's restatement: models of 0, 1 and 2 spheres, all spheres on one link, the adjacency flag with and
without `parent`, ignored link pairs in either order, a capacity below the count, and each error message."""
import ctypes

import numpy as np
import pytest

import kinematics_cases
import self_ref as R
from voxelized_geometry_tools_amd import capi


def both(link, num_links, **kw):
    got, count = capi.self_collision_pairs(link, num_links, **kw)
    want = R.self_collision_pairs(link, num_links, **kw)
    assert got.dtype == np.int32 and got.shape == want.shape and count == len(want)
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("link", [[], [0], [2], [0, 1], [1, 1], [1, 0]])
def test_models_of_at_most_two_spheres(link):
    got = both(link, 3)
    assert len(got) == (1 if len(link) == 2 and link[0] != link[1] else 0)
    both(link, 3, parent=[-1, 0, 1], skip_adjacent=True, ignored_link_pairs=[[0, 2]])


def test_all_spheres_on_one_link():
    assert len(both([4] * 9, 5)) == 0


@pytest.mark.parametrize("name", ["arm", "body"])
def test_trees_with_the_adjacency_flag_and_ignored_pairs(name):
    tree = kinematics_cases.tree(name)
    _, link = kinematics_cases.sphere_model(tree, 40, 11)
    everything = both(link, tree.num_links)
    assert (everything[:, 0] < everything[:, 1]).all()
    assert everything.tolist() == sorted(everything.tolist())                   # lexicographic
    # the flag without `parent` changes nothing; with it parents and children go
    assert len(both(link, tree.num_links, skip_adjacent=True)) == len(everything)
    assert len(both(link, tree.num_links, parent=tree.parent)) == len(everything)
    apart = both(link, tree.num_links, parent=tree.parent, skip_adjacent=True)
    assert 0 < len(apart) < len(everything)
    for a, b in apart:
        assert tree.parent[link[a]] != link[b] and tree.parent[link[b]] != link[a]
    # ignored pairs, unordered: either order and a repeated row give the same list
    ignored = [[int(link[0]), int(link[-1])], [2, 0], [1, 1]]
    first = both(link, tree.num_links, ignored_link_pairs=ignored)
    second = both(link, tree.num_links, ignored_link_pairs=[row[::-1] for row in ignored] + [[0, 2]])
    assert np.array_equal(first, second) and len(first) < len(everything)
    both(link, tree.num_links, parent=tree.parent, skip_adjacent=True, ignored_link_pairs=ignored)


def test_capacity_below_the_count():
    link = [0, 1, 2, 0, 1]
    want = R.self_collision_pairs(link, 3)
    for capacity in (0, 1, len(want) - 1, len(want), len(want) + 3):
        got, count = capi.self_collision_pairs(link, 3, capacity=capacity)
        assert count == len(want) and np.array_equal(got, want[:capacity])
    # through the C ABI: nothing is written behind the capacity, and NULL with capacity 0 only counts
    lib = capi.load()
    out = np.full((len(want) + 2, 2), 77, np.int32)
    count = ctypes.c_int64(-1)
    sphere_link = np.asarray(link, np.int32)
    assert lib.vgt_hip_self_collision_pairs(capi._ptr(sphere_link), 5, None, 3, None, 0, 0, capi._ptr(out), 3,
                                            ctypes.byref(count)) == 0
    assert count.value == len(want) and np.array_equal(out[:3], want[:3]) and (out[3:] == 77).all()
    count = ctypes.c_int64(-1)
    assert lib.vgt_hip_self_collision_pairs(capi._ptr(sphere_link), 5, None, 3, None, 0, 0, None, 0,
                                            ctypes.byref(count)) == 0 and count.value == len(want)


def test_error_messages():
    link = [0, 1, 2, 0]
    with pytest.raises(ValueError, match=r"sphere 2: link 3 is not in \[0, num_links\)"):
        capi.self_collision_pairs([0, 1, 3, 5], 3)
    with pytest.raises(ValueError, match=r"sphere 1: link -1 is not in \[0, num_links\)"):
        capi.self_collision_pairs([0, -1, 3], 3)
    with pytest.raises(ValueError, match=r"link 1: parent 3 is not in \[-1, num_links\)"):
        capi.self_collision_pairs(link, 3, parent=[-1, 3, -2])
    with pytest.raises(ValueError, match=r"link 2: parent -2 is not in \[-1, num_links\)"):
        capi.self_collision_pairs(link, 3, parent=[-1, 0, -2])
    with pytest.raises(ValueError, match=r"ignored pair 1: link 3 is not in \[0, num_links\)"):
        capi.self_collision_pairs(link, 3, ignored_link_pairs=[[0, 1], [3, -1]])
    with pytest.raises(ValueError, match=r"ignored pair 0: link -1 is not in \[0, num_links\)"):
        capi.self_collision_pairs(link, 3, ignored_link_pairs=[[2, -1]])
    lib = capi.load()
    sphere_link = np.asarray(link, np.int32)
    count = ctypes.c_int64(-1)

    def refused(needle, link_ptr=capi._ptr(sphere_link), spheres=4, links=3, ignored=None, num_ignored=0, flags=0,
                out=None, capacity=0, count_ref=ctypes.byref(count)):
        rc = lib.vgt_hip_self_collision_pairs(link_ptr, spheres, None, links, ignored, num_ignored, flags, out, capacity,
                                              count_ref)
        message = lib.vgt_hip_last_error()
        assert rc == 1 and needle in message, (rc, message)

    refused(b"null", count_ref=None)
    refused(b"null", link_ptr=None)
    refused(b"null", num_ignored=1)
    refused(b"null", capacity=1)
    refused(b"must not be negative", spheres=-1)
    refused(b"must not be negative", links=-1, spheres=0)
    refused(b"must not be negative", capacity=-1)
    refused(b"unknown self-collision pair flag", flags=2)
    assert count.value == -1
