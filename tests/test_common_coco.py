"""popnet_amd.utils.common_coco.Human: the pair-based assembly surface of tpm/lib/utils/common_coco.py:27-60 (CPU; data only)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from popnet_amd.utils.common_coco import BodyPart, Human  # noqa: E402


class Pair:
    def __init__(self, p1, i1, c1, p2, i2, c2, score):
        self.part_idx1, self.idx1, self.coord1 = p1, i1, c1
        self.part_idx2, self.idx2, self.coord2 = p2, i2, c2
        self.score = score


PAIRS = [Pair(1, 0, (0.5, 0.25), 2, 3, (0.4, 0.3), 0.9), Pair(2, 3, (0.4, 0.3), 3, 1, (0.35, 0.45), 0.7),
         Pair(1, 1, (0.8, 0.2), 5, 0, (0.9, 0.3), 0.6), Pair(5, 0, (0.9, 0.3), 6, 2, (0.95, 0.5), 0.8), Pair(3, 1, (0.35, 0.45), 4, 4, (0.3, 0.6), 0.5)]


def _state(h):
    return (sorted(h.uidx_list), {k: (v.uidx, v.part_idx, v.x, v.y, v.score) for k, v in h.body_parts.items()}, len(h.pairs), h.score)


def test_pair_constructor_and_methods():
    a = Human(PAIRS[:2])
    assert a.part_count() == 3 and sorted(a.uidx_list) == ["1-0", "2-3", "3-1"] and a.score == 0.0
    assert a.body_parts[2].score == 0.7 and a.body_parts[2].uidx == "2-3"          # the later pair's end point replaces the earlier one's
    assert a.body_parts[1].x == 0.5 and a.body_parts[3].y == 0.45 and a.get_max_score() == 0.9
    b = Human(PAIRS[2:4])
    assert not a.is_connected(b) and not b.is_connected(a)
    c = Human([PAIRS[4]])
    assert a.is_connected(c) and c.is_connected(a) and not b.is_connected(c)
    a.merge(c)
    assert a.part_count() == 4 and len(a.pairs) == 3 and "4-4" in a.uidx_list and a.body_parts[3].score == 0.5
    e = Human([])
    assert e.part_count() == 0 and e.pairs == [] and e.uidx_list == set()
    e.body_parts[0] = BodyPart("0-0", 0, 0.1, 0.2, 0.3)                           # how paf_to_pose_cpp fills it
    assert e.get_max_score() == 0.3


def _json_state(h):
    """_state in the JSON shape tests/golden/make_golden.py stores (golden_common_coco)."""
    return [sorted(h.uidx_list), [[k, v.uidx, v.part_idx, v.x, v.y, v.score] for k, v in sorted(h.body_parts.items())], len(h.pairs), h.score]


def test_same_states_as_the_reference_class():
    """Every constructor / merge / is_connected outcome against the reference's own class, on the same pairs: its outcomes for every
    split of PAIRS are stored in tests/golden/common_coco.json (make_golden.py step common_coco)."""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "common_coco.json")))
    assert g["pairs"] == [[p.part_idx1, p.idx1, list(p.coord1), p.part_idx2, p.idx2, list(p.coord2), p.score] for p in PAIRS]
    assert [r["split"] for r in g["splits"]] == list(range(len(PAIRS) + 1))
    for r in g["splits"]:
        split = r["split"]
        mine, m2 = Human(PAIRS[:split]), Human(PAIRS[split:])
        assert _json_state(mine) == r["first"] and _json_state(m2) == r["second"]
        assert mine.is_connected(m2) == r["connected"]
        mine.merge(m2)
        assert _json_state(mine) == r["merged"] and mine.part_count() == r["merged_part_count"]
        if mine.body_parts:
            assert mine.get_max_score() == r["merged_max_score"]
