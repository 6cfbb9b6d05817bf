"""Markers, poses and states for the tests of the map-object markers on the map frames (test_map_things_host.py, test_map_things_gpu.py),
on floor_map_cases' worlds `light` (synth:1993, 40 map objects) and `hand` (two imps and two barrels).

A case is a floor_map_cases case (world, view, timestamp, scale, flags, mask) with:
   marked    {object: (radius, rgb, flags)}: the marker table has these, every other object (0, 0, 0) — no marker
   poses     the view's dg_view_poses entries [(mobj, x, y, angle)], in order (the later of two wins)
   mobjs     the view's dg_mobj_state entries [(mobj, sprite_frame, full_bright)], in order
   shown     the objects the rule shows in this view — what the case is about; the model derives it again on its own
A case is POSITIVE when `shown` is not empty: its view and scale are chosen so that every shown marker lies in a 64x48 frame, and
test_map_things_host.py asserts on the model that each of them keeps a pixel no later line covers.
"""
import math

import numpy as np

import floor_map_cases as fc
import np_map_things as nt

F = np.float32
R, A = fc.R, fc.A
BOX, HEADING = nt.BOX, nt.HEADING
SIZES = [(64, 48), (333, 77), (16, 16)]


def rgb_of(i: int) -> int:
    """A colour of object i's own: never the map's red or yellow, never black."""
    return 0x80 | (((91 * i + 60) & 255) << 8) | (((37 * i + 80) & 255) << 16)


def things_of(world: str):
    return nt.read_things(fc.wad_of(world))


def table(world: str, marked: dict):
    """The whole marker table [(radius, rgb, flags)] of a case."""
    n = len(things_of(world))
    return [tuple(marked.get(i, (0, 0, 0))) for i in range(n)]


def default_table(world: str):
    """Every object marked: radii 8 .. 24, the three flag combinations, and every seventh object without a marker."""
    n = len(things_of(world))
    return [(8 + 8 * (i % 3), rgb_of(i), 0 if i % 7 == 3 else (BOX | HEADING, BOX, HEADING)[i % 3]) for i in range(n)]


def case(name, world, x, y, angle, scale, flags, marked, shown, mask=None, poses=(), mobjs=(), ts=0.0):
    c = fc.case(name, world, x, y, angle, ts, scale, flags, mask)
    c.update(marked=dict(marked), poses=[tuple(p) for p in poses], mobjs=[tuple(m) for m in mobjs], shown=set(shown))
    return c


def hidden_of(c, scene_hidden=()):
    """The objects whose composed sprite frame is -1: the view's later entry, else the scene's."""
    out = set(scene_hidden)
    for m, (sf, _fb) in nt.latest(c["mobjs"]).items():
        (out.add if sf < 0 else out.discard)(m)
    return out


def model_lines(c, W, H, scene_hidden=()):
    return nt.thing_lines(W, H, fc.na.libm_view(*c["view"]), c["scale"], c["flags"], things_of(c["world"]), table(c["world"], c["marked"]), hidden_of(c, scene_hidden), c["poses"])


def model_ego(c, W, H, row=0, scene_hidden=()):
    return nt.ego_frame(fc.model_of(c["world"]).ego, W, H, fc.na.libm_view(*c["view"]), c["scale"], c["flags"], fc.mask_row(c, row), model_lines(c, W, H, scene_hidden))


def model_floor(c, W, H, row=0, scene_hidden=()):
    return nt.floor_frame(fc.model_frame(c, W, H, row), fc.model_of(c["world"]).ego, W, H, fc.na.libm_view(*c["view"]), c["scale"], c["flags"], fc.mask_row(c, row),
                          model_lines(c, W, H, scene_hidden))


def state_of(c):
    """(lights, mobjs) as make_view_states takes it, or None."""
    return ([], list(c["mobjs"])) if c["mobjs"] else None


def poses_of(c):
    return list(c["poses"]) if c["poses"] else None


def _near(world, k, count):
    """Object k and its count - 1 nearest neighbours."""
    th = things_of(world)
    d = sorted(range(len(th)), key=lambda i: (float(th[i][0]) - float(th[k][0])) ** 2 + (float(th[i][1]) - float(th[k][1])) ** 2)
    return d[:count]


def _cases():
    out = []
    hand = things_of("hand")                                                   # imps at (600, 250) and (250, 300), barrels at (200, 120) and (700, 120)
    assert len(hand) == 4
    both = BOX | HEADING
    h_marked = {0: (20, rgb_of(0), both), 1: (16, rgb_of(1), both), 2: (12, rgb_of(2), BOX), 3: (0, 0, 0)}
    # the whole hand world in the frame, north-up and rotated, with and without mask and arrow
    for k, (flags, mask) in enumerate(((0, None), (R, None), (A, ("lines", (0, 1, 2))), (R | A, ("ones",)), (R, ("zero",)))):
        out.append(case(f"hand_whole_{k}", "hand", 352.5, 250.0, 0.1 + 0.7 * k, 0.05, flags, h_marked, {0, 1, 2}, mask))
    out.append(case("hand_unit", "hand", 590.0, 262.0, 0.4, 1.0, R | A, {0: (10, rgb_of(0), both)}, {0}))
    # the light world: an object and its neighbours, the view between them
    light = things_of("light")
    for n, k in enumerate((0, 7, 19, 33)):
        near = _near("light", k, 3)
        cx = float(np.mean([float(light[i][0]) for i in near])) + 0.5
        cy = float(np.mean([float(light[i][1]) for i in near])) - 0.25
        far = max(max(abs(float(light[i][0]) - cx), abs(float(light[i][1]) - cy)) for i in near) + 24.0
        scale = min(1.0, 2.0 ** math.floor(math.log2(20.0 / far)))
        marked = {i: (8 + 8 * (j % 3), rgb_of(i), (both, BOX, HEADING)[(n + j) % 3]) for j, i in enumerate(near)}
        out.append(case(f"light_near_{k}", "light", cx, cy, 0.3 + n, scale, (0, R, A, R | A)[n], marked, set(near), ("half", 5) if n == 1 else None))
    # later pose wins: the imp is where its second entry puts it, with that entry's angle
    out.append(case("later_pose_wins", "hand", 352.5, 250.0, 0.0, 0.05, 0, {0: (20, rgb_of(0), both)}, {0}, poses=[(0, 100.0, 100.0, 0.0), (1, 0.0, 0.0, 0.0), (0, 500.5, 320.25, 2.5)]))
    # hidden by a state entry of -1; shown again by a later entry
    out.append(case("state_entry_hides", "hand", 352.5, 250.0, 0.0, 0.05, A, h_marked, {1, 2}, mobjs=[(0, -1, 0)]))
    out.append(case("later_state_entry_shows", "hand", 352.5, 250.0, 0.0, 0.05, A, h_marked, {0, 1, 2}, mobjs=[(0, -1, 0), (0, 0, 1)]))
    # positions at the edge of the rule: 32768.0 is drawn, 32768.5, NaN and an infinity are not
    edge = {0: (16, rgb_of(0), both), 1: (16, rgb_of(1), both), 2: (16, rgb_of(2), both)}
    out.append(case("pose_at_32768", "hand", 32760.0, 32750.0, 0.0, 1.0, R, edge, {0}, poses=[(0, 32768.0, 32768.0, 1.0), (1, 32768.5, 32760.0, 0.0), (2, float("nan"), 32760.0, 0.0)]))
    out.append(case("pose_beyond", "hand", 32760.0, -32750.0, 0.0, 1.0, 0, edge, set(), poses=[(0, 32760.0, -32768.5, 1.0), (1, float("inf"), 0.0, 0.0), (2, 32760.0, float("nan"), 0.0)]))
    # an angle that is not finite: the box alone
    out.append(case("heading_not_finite", "hand", 352.5, 250.0, 0.0, 0.05, 0, h_marked, {0, 1, 2}, poses=[(0, 600.0, 250.0, float("nan")), (1, 250.0, 300.0, float("inf"))]))
    # radius 0: the box is one point, the heading too
    out.append(case("radius_0", "hand", 590.0, 262.0, 0.4, 1.0, R, {0: (0, rgb_of(0), both)}, {0}))
    # a marker over a line and under the arrow: the barrel moved onto the vertex a0 where two walls meet, the player on its box's top edge
    out.append(case("over_a_line_under_the_arrow", "hand", 0.0, 12.0, 0.0, 1.0, A, {2: (12, rgb_of(2), both)}, {2}, poses=[(2, 0.0, 0.0, 0.0)]))
    # an object exactly at the player
    out.append(case("at_the_player", "hand", 600.0, 250.0, 2.0, 2.0, R | A, {0: (8, rgb_of(0), both)}, {0}))
    # a black marker: on a floor-textured frame its pixels stay black
    out.append(case("black_marker", "hand", 590.0, 262.0, 0.4, 1.0, 0, {0: (10, 0, BOX)}, {0}))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
