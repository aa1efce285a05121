"""The flight model's arena has a compile-time layout (dev_model.hpp, lay::): the step kernel reads every table at arena + constant,
everything else through the struct's pointer fields.  tests/flight_layout_host.cpp - the host table builder as a stand-alone program under
AddressSanitizer and UBSan, never loaded into Python - builds the arena from the shipped blob and from a blob without collision geoms,
and reports each table as seen both ways."""
import os
import subprocess

import pytest

from conftest import ROOT

BLOB = os.path.join(ROOT, "flybody_amd", "assets", "fly_flight.ffmb")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("flight_layout") / "flight_layout_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path,
                           os.path.join(ROOT, "tests", "flight_layout_host.cpp")])
    return path


def run(exe, blob):
    r = subprocess.run([exe, blob], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    tables, keys = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "table":
            tables[f[1]] = dict(zip(("off", "cap", "count", "esize", "bad", "dirty"), map(int, f[2:])))
        else:
            keys[f[0]] = int(f[1])
    return tables, keys


@pytest.fixture(scope="module")
def shipped(exe):
    return run(exe, BLOB)


@pytest.fixture(scope="module")
def no_geoms(exe, tmp_path_factory):
    """The shipped model without its collision geoms and candidate pairs: the builder's ncg == 0 branch."""
    from flybody_amd.model import blob

    t = {k: v for k, v in blob.read_blob(BLOB).items() if not (k.startswith("cgeom_") or k.startswith("cand_"))}
    path = str(tmp_path_factory.mktemp("flight_layout_blob") / "fly_flight_nogeom.ffmb")
    blob.write_blob(path, t)
    return run(exe, path)


def check_layout(tables, keys):
    assert keys["tables"] + 1 == len(tables) and keys["tables"] >= 70, (keys["tables"], len(tables))
    assert keys["struct_bytes"] <= keys["header"], keys
    assert keys["arena_field"] == 1
    assert keys["header_nonzero"] == 0, "the builder leaves the struct's place empty"
    spans = sorted((t["off"], t["off"] + t["cap"], name) for name, t in tables.items())
    assert spans[0][0] >= keys["header"], spans[0]
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, f"{an} [{a0}, {a1}) overlaps {bn} [{b0}, {b1})"
    for name, t in tables.items():
        assert t["off"] % keys["align"] == 0 and keys["align"] == 256, (name, t)
        assert t["off"] + t["cap"] <= keys["arena_bytes"], (name, t, keys["arena_bytes"])
        assert t["count"] * t["esize"] == t["cap"], (name, t)
        assert t["bad"] == 0, f"{name}: {t['bad']} elements differ between the pointer field and arena + offset"
        assert t["dirty"] == 0, (name, t)
    assert spans[-1][2] == "fsched", "the table of open length is the tail"
    assert keys["solve_dims"] == keys["nv"] | (keys["nroot"] << 8) | (keys["nbr_steps"] << 16)
    assert keys["content_wrong"] == 0


def test_fixed_offsets_address_what_the_pointer_fields_address(shipped):
    tables, keys = shipped
    check_layout(tables, keys)
    assert (keys["nv"], keys["nq"], keys["nlink"], keys["nM"]) == (42, 43, 19, 421), keys
    assert keys["ncg"] == 70 and 0 < keys["ncp"] <= 384, keys


def test_layout_of_a_model_without_geoms(no_geoms, shipped):
    tables, keys = no_geoms
    check_layout(tables, keys)
    assert keys["ncg"] == 0 and keys["ncp"] == 0, keys
    # the layout is the kernel's, not the model's: the same offsets, and the same arena up to the collision tables
    assert {n: (t["off"], t["cap"]) for n, t in tables.items()} == {n: (t["off"], t["cap"]) for n, t in shipped[0].items()}
    assert keys["arena_bytes"] == shipped[1]["arena_bytes"]
