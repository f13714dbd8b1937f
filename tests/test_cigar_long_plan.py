"""CPU: tredparse_amd/csrc/cigar_long_plan.h, the slot and workspace planning of sw_cigar_long.hip, through the stand-alone
driver tests/cigar_long_plan_main.cpp built with the address and undefined-behaviour sanitizers: the bytes of a rectangle,
the 1 GiB cap and the order in which the slots take the items."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SLOTS, CAP, ALIGN = 256, 1 << 30, 256


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cigar_long_plan") / "cigar_long_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "cigar_long_plan_main.cpp")])

    def call(*args):
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr        # the sanitizers report nothing
        return r.stdout.splitlines()
    return call


def up(n):
    return max(ALIGN, -(-n // ALIGN) * ALIGN)


def test_slot_count_matches_the_binding():
    from tredparse_amd import _lib
    src = open(os.path.join(HERE, "..", "tredparse_amd", "csrc", "cigar_long_plan.h")).read()
    assert "constexpr int SLOTS = {};".format(_lib.LONG_CIGAR_SLOTS) in src and _lib.LONG_CIGAR_SLOTS == SLOTS


@pytest.mark.parametrize("fields,want", [
    ((0, 0, 0, 0), 1), ((0, 4094, 0, 2047), 4095 * 2048), ((5, 704, 2, 601), 700 * 600), ((100, 100, 7, 7), 1),
    ((0, 4095, 0, 10), 0), ((0, 10, 0, 2048), 0),                      # beyond the limits: refused before a pass
    ((-1, 10, 0, 10), 0), ((0, 10, -1, 10), 0), ((11, 10, 0, 10), 0), ((0, 10, 11, 10), 0),
    ((-32768, 32767, 0, 10), 0), ((0, 32767, 0, 32767), 0), ((32767, 32767, 32767, 32767), 0),
])
def test_rectangle_bytes(run, fields, want):
    assert run("R", *fields) == [str(want)]


def test_plan_is_sized_from_the_largest_rectangle(run):
    assert run("P") == ["{} 0 0".format(ALIGN)]                       # no items: no wavefront
    assert run("P", 1, 0, 0, 0, 0) == ["{} 1 {}".format(ALIGN, ALIGN)]
    assert run("P", 3, 0, 699, 0, 599, 1, 0, 99, 0, 99) == ["{} 4 {}".format(up(420000), 4 * up(420000))]
    assert run("P", 1000, 0, 699, 0, 599) == ["{} {} {}".format(up(420000), SLOTS, SLOTS * up(420000))]
    # a refused item asks for nothing
    assert run("P", 2, 0, 99, 0, 99, 1, 0, 4095, 0, 2047, 1, -1, 5, 0, 5) == ["{} 4 {}".format(up(10000), 4 * up(10000))]


def test_the_cap_takes_slots_away_not_bytes(run):
    big = 4095 * 2048
    assert big % ALIGN == 0
    slots = CAP // big
    assert slots == 128 < SLOTS
    assert run("P", 1000, 0, 4094, 0, 2047) == ["{} {} {}".format(big, slots, slots * big)]
    assert slots * big <= CAP < (slots + 1) * big
    # one large item among small ones sizes every slot
    assert run("P", 1, 0, 4094, 0, 2047, 999, 0, 9, 0, 9) == ["{} {} {}".format(big, slots, slots * big)]
    assert run("P", 3, 0, 4094, 0, 2047) == ["{} 3 {}".format(big, 3 * big)]
    # the largest rectangle at which all 256 slots still fit: 4 MiB each
    assert run("P", 300, 0, 2047, 0, 2047) == ["{} {} {}".format(2048 * 2048, SLOTS, CAP)]
    assert run("P", 300, 0, 2048, 0, 2047) == ["{} {} {}".format(up(2049 * 2048), CAP // up(2049 * 2048), CAP // up(2049 * 2048) * up(2049 * 2048))]


def test_slots_take_items_in_turn(run):
    out = run("O", 10, 4, "O", 5, 1, "O", 3, 256)
    assert out[0].split() == ["0:0", "1:0", "2:0", "3:0", "0:1", "1:1", "2:1", "3:1", "0:2", "1:2"]
    assert out[1].split() == ["0:{}".format(k) for k in range(5)]
    assert out[2].split() == ["0:0", "1:0", "2:0"]
