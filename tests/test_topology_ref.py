"""(not gpu) The two CPU yardsticks of the component topology (tests/topology_ref.py) give the known answers and agree
with each other on every hand case and on the random small grids the GPU tests use."""
import numpy as np

import components_ref as R
import topology_ref as T


def test_c_division():
    assert [T.trunc_div(a, 8) for a in (-9, -8, -6, -1, 0, 7, 8, 15)] == [-1, -1, 0, 0, 0, 0, 1, 1]


def test_known_answers_hold_for_both_yardsticks():
    for name, occ, want in T.known_answer_cases():
        occ, labels, count = T.labelled(occ)
        for table in (T.topology_literal(occ, labels, 7, count), T.topology_fast(occ, labels, 7, count)):
            assert len(table) == count + 1 and not any(table[0][f] for f in T.FIELDS), name
            for cell, (holes, voids) in want.items():
                entry = table[labels[cell]]
                assert entry["present"] == 1 and (entry["num_holes"], entry["num_voids"]) == (holes, voids), (name, cell)
    # the counts behind two of them: a cube has 8 corners; a slab with a hole 8 convex and 8 concave-edge vertices
    occ, labels, count = T.labelled(T.known_answer_cases()[0][1])
    cube = T.topology_fast(occ, labels, 7, count)[labels[3, 3, 3]]
    assert (cube["m3"], cube["m5"], cube["m6"]) == (8, 0, 0)
    occ, labels, count = T.labelled(T.known_answer_cases()[1][1])
    slab = T.topology_fast(occ, labels, 7, count)[labels[2, 2, 2]]
    assert (slab["m3"], slab["m5"], slab["m6"]) == (8, 8, 0)


def test_class_selection():
    occ = np.zeros((5, 5, 5), np.float32)
    occ[1:4, 1:4, 1:4] = 0.5
    occ[2, 2, 2] = 1.0
    occ[0, 0, 0] = np.nan          # NaN is "unknown" for the selection, a component of its own for the labelling
    occ, labels, count = T.labelled(occ)
    assert count == 4
    bits = {int(labels[0, 0, 0]): 4, int(labels[0, 0, 1]): 2, int(labels[1, 1, 1]): 4, int(labels[2, 2, 2]): 1}
    for types in range(1, 8):
        for table in (T.topology_literal(occ, labels, types, count), T.topology_fast(occ, labels, types, count)):
            for c, bit in bits.items():
                assert table[c]["present"] == (1 if types & bit else 0), (types, c)
                if not types & bit:
                    assert not any(table[c][f] for f in T.FIELDS)


def test_literal_equals_fast_on_the_hand_cases_and_random_grids():
    cases = [(occ, ids) for _, occ, ids in T.hand_cases()] + R.random_small_grids(200)
    assert len(cases) >= 212
    remainders = shared = 0
    for k, (occ, ids) in enumerate(cases):
        # (alternating: components by class, and by class and object id, as the tagged map labels them)
        occ, labels, count = T.labelled(occ, ids if k % 2 else None)
        types = 7 if k % 3 else 1 + k % 7
        fast = T.topology_fast(occ, labels, types, count)
        assert T.tables_equal(T.topology_literal(occ, labels, types, count), fast), (k, occ.shape, types)
        remainders += int(np.sum((fast["m5"] + 2 * fast["m6"] - fast["m3"]) % 8 != 0))
        vertex = T.vertex_label_pairs(occ, labels, types, count)[0]
        if vertex.size:
            shared += int(np.sum(np.unique(vertex, return_counts=True)[1] >= 3))
    # the set must keep exercising C's division of a numerator with a remainder, and vertices that several components share
    assert remainders >= 1 and shared >= 1


def test_pinched_pair_has_a_remainder_that_tells_c_division_from_floor_division():
    occ = dict((name, occ) for name, occ, _ in T.known_answer_cases())["pinched_pair"]
    occ, labels, count = T.labelled(occ)
    entry = T.topology_fast(occ, labels, 7, count)[labels[1, 1, 1]]
    numerator = int(entry["m5"]) + 2 * int(entry["m6"]) - int(entry["m3"])
    assert numerator % 8 != 0 and numerator < 0
    assert entry["num_holes"] == 1 + T.trunc_div(numerator, 8) + entry["num_voids"] != 1 + numerator // 8 + entry["num_voids"]
