"""CPU: the HDF5 writer (anatomix_amd/io/hdf5_write.py).  What it writes is read back through the pinned reader (io/hdf5.py) and,
where the build container's h5py interpreter exists, by the real library in a subprocess: every object is visited, every dataset
compared bit for bit, ``keys()`` orders compared, and the same arrays written by h5py the reference's way give identical content
through this project's reader."""
import os
import subprocess
import sys

import numpy as np
import pytest

from anatomix_amd.io import H5File
from anatomix_amd.io.hdf5_write import H5Writer

H5PY_PYTHON = "/opt/conda/bin/python3.9"
GROUP_SIZES = [0, 1, 8, 9, 256, 257, 2000]       # one symbol-table node, a split, a full B-tree node (32 x 8), two levels, three
DTYPES = ["u1", "<i2", "<i8", "<f2", "<f4", "<f8", ">u2", ">f4"]


def _walk(group, prefix=""):
    """{path: array} of every dataset below ``group`` and [(path, keys)] of every group, through this project's reader."""
    data, groups = {}, [(prefix or "/", list(group.keys()))]
    for k in group.keys():
        node = group[k]
        if hasattr(node, "keys"):
            d, g = _walk(node, prefix + "/" + k)
            data.update(d)
            groups += g
        else:
            data[prefix + "/" + k] = node[...]
    return data, groups


def _check(path, expect):
    """Every dataset of ``expect`` {path: array} reads back equal, with its dtype, and every group lists its names in order."""
    with H5File(str(path)) as f:
        data, groups = _walk(f)
    assert sorted(data) == sorted(expect)
    for k, a in expect.items():
        assert data[k].dtype == a.dtype and data[k].shape == a.shape and np.array_equal(data[k], a), k
    for _, keys in groups:
        assert keys == sorted(keys)
    return data, groups


def write_reference_layout(path, rng):
    expect = {}
    with H5Writer(path) as f:
        for i, shape in enumerate([(12, 10, 8), (9, 11, 7), (12, 10, 8)]):
            grp = f.create_group("{:06}".format(i))
            img = rng.randint(0, 256, (2,) + shape).astype(np.uint8)
            seg = rng.randint(0, 40, shape).astype(np.uint8)
            grp["img"] = img
            grp["seg"] = seg
            expect["/%06d/img" % i], expect["/%06d/seg" % i] = img, seg
    return expect


def write_variants(path, rng):
    expect = {}
    with H5Writer(path) as f:
        a = f.create_group("a")
        b = a.create_group("b")
        c = f.create_group("x/y/z")                       # intermediate groups, as h5py makes them
        assert f["x"]["y"]["z"] is c and f["a/b"] is b
        for where, grp in (("/a", a), ("/a/b", b), ("/x/y/z", c), ("", f)):
            for dt in DTYPES:
                arr = (rng.randn(3, 5, 2) * 50).astype(dt)
                grp["d" + dt.strip("<>") + ("be" if dt[0] == ">" else "")] = arr
                expect[where + "/d" + dt.strip("<>") + ("be" if dt[0] == ">" else "")] = arr
            for dt in ("u1", "<f4", ">f4", "<i8"):
                arr = np.array(rng.randint(1, 100), dtype=dt)
                grp["scalar_" + dt.strip("<>") + ("be" if dt[0] == ">" else "")] = arr
                expect[where + "/scalar_" + dt.strip("<>") + ("be" if dt[0] == ">" else "")] = arr
        f["strided"] = np.arange(24, dtype=np.int16).reshape(4, 6)[:, ::2]
        expect["/strided"] = np.arange(24, dtype=np.int16).reshape(4, 6)[:, ::2].copy()
        f["empty_array"] = np.zeros((0, 3), np.float32)
        expect["/empty_array"] = np.zeros((0, 3), np.float32)
        f.create_group("hollow")
    return expect


def write_many(path, n):
    """A root of n groups (named so that creation order is not name order) each with one small dataset, and a group of n datasets."""
    expect = {}
    names = ["%06d" % ((i * 7919) % (n + 13)) + "_%d" % i for i in range(n)]
    with H5Writer(path) as f:
        flat = f.create_group("flat")
        for i, name in enumerate(names):
            f.create_group(name)["v"] = np.array([i, -i], np.int32)
            expect["/" + name + "/v"] = np.array([i, -i], np.int32)
            flat[name] = np.uint8(i % 251)
            expect["/flat/" + name] = np.array(i % 251, np.uint8)
    return expect


def test_round_trip_reference_layout(tmp_path):
    p = tmp_path / "train_data.hdf5"
    expect = write_reference_layout(p, np.random.RandomState(0))
    _, groups = _check(p, expect)
    assert groups[0] == ("/", ["000000", "000001", "000002"]) and groups[1][1] == ["img", "seg"]
    with H5File(str(p)) as f:
        assert f["000001"]["img"].shape == (2, 9, 11, 7) and f["000001/seg"].dtype == np.uint8
        assert np.array_equal(f["000002"]["img"][1], expect["/000002/img"][1])
        raw = open(p, "rb").read()
    assert int.from_bytes(raw[40:48], "little") == len(raw)           # the superblock's end-of-file address is the file length


def test_round_trip_nested_groups_and_types(tmp_path):
    p = tmp_path / "variants.hdf5"
    expect = write_variants(p, np.random.RandomState(1))
    _, groups = _check(p, expect)
    assert dict(groups)["/hollow"] == [] and dict(groups)["/x/y"] == ["z"]


@pytest.mark.parametrize("n", GROUP_SIZES)
def test_many_links(tmp_path, n):
    p = tmp_path / "many.hdf5"
    expect = write_many(p, n)
    _, groups = _check(p, expect)
    assert len(dict(groups)["/"]) == n + 1 and len(dict(groups)["/flat"]) == n
    raw = open(p, "rb").read()
    # nodes occupy their full size: every B-tree node is followed by 544 bytes that belong to it, every symbol-table node by 328
    for sig, size in ((b"TREE", 544), (b"SNOD", 328)):
        at = raw.find(sig)
        while at >= 0:
            assert at % 8 == 0 and at + size <= len(raw)
            at = raw.find(sig, at + size)


def test_writer_refusals(tmp_path):
    p = tmp_path / "r.hdf5"
    with H5Writer(p) as f:
        g = f.create_group("g")
        g["x"] = np.zeros(3, np.uint8)
        for bad in (np.array(["a", "b"]), np.array([b"ab"]), np.array([object()], dtype=object), np.zeros(2, np.complex64),
                    np.zeros(2, bool), np.zeros(2, [("a", "u1")])):
            with pytest.raises(NotImplementedError, match="dtype"):
                g["bad"] = bad
        assert "bad" not in g
        with pytest.raises(ValueError, match="already exists"):
            g["x"] = np.zeros(3, np.uint8)
        with pytest.raises(ValueError, match="already exists"):
            f.create_group("g")
        with pytest.raises(ValueError, match="already exists"):
            g.create_group("x")
        with pytest.raises(ValueError):
            g["a/b"] = np.zeros(1)
    _check(p, {"/g/x": np.zeros(3, np.uint8)})
    with pytest.raises(ValueError, match="closed"):
        g["y"] = np.zeros(3, np.uint8)
    with pytest.raises(ValueError, match="closed"):
        f.create_group("h")
    with pytest.raises(ValueError):
        H5File(str(p), "w")                                           # the reader stays read-only
    _check(p, {"/g/x": np.zeros(3, np.uint8)})


def test_exception_leaves_no_file(tmp_path):
    p = tmp_path / "partial.hdf5"
    with pytest.raises(RuntimeError, match="boom"):
        with H5Writer(p) as f:
            f.create_group("g")["x"] = np.arange(1000)
            assert p.exists()
            raise RuntimeError("boom")
    assert not p.exists()
    with pytest.raises(NotImplementedError):
        with H5Writer(p) as f:
            f["s"] = np.array(["text"])
    assert not p.exists()


_H5PY_SCRIPT = r"""
import sys
import h5py
import numpy as np
out = {}
for tag, path in zip(sys.argv[2::2], sys.argv[3::2]):
    with h5py.File(path, "r") as f:
        seen = []
        f.visititems(lambda name, obj: seen.append((name, obj)))
        for name, obj in seen:
            if isinstance(obj, h5py.Dataset):
                a = obj[()]
                out[tag + ":d:/" + name] = np.asarray(a)
                out[tag + ":t:/" + name] = np.array(obj.dtype.str)
            else:
                out[tag + ":k:/" + name] = np.array(list(obj.keys()), dtype="U")
        out[tag + ":k:/"] = np.array(list(f.keys()), dtype="U")
        # the same arrays written the reference's way (grp[name] = array)
        with h5py.File(path + ".h5py", "w") as g:
            for name, obj in seen:
                if isinstance(obj, h5py.Group):
                    g.create_group(name)
            for name, obj in seen:
                if isinstance(obj, h5py.Dataset):
                    parent, _, leaf = name.rpartition("/")
                    (g[parent] if parent else g)[leaf] = np.asarray(obj[()], dtype=obj.dtype)      # (a scalar comes back native)
np.savez(sys.argv[1], **out)
print("h5py", h5py.__version__, "hdf5", h5py.version.hdf5_version, "opened", len(sys.argv[2::2]), "files")
"""


def _h5py_available():
    if not os.path.exists(H5PY_PYTHON):
        return False
    return subprocess.run([H5PY_PYTHON, "-c", "import h5py"], capture_output=True).returncode == 0


def test_real_library_reads_what_the_writer_wrote(tmp_path):
    if not _h5py_available():
        pytest.skip(f"{H5PY_PYTHON} with h5py is absent")
    rng = np.random.RandomState(2)
    files = {"layout": (tmp_path / "layout.hdf5", write_reference_layout), "variants": (tmp_path / "variants.hdf5", write_variants)}
    expect = {tag: fn(p, rng) for tag, (p, fn) in files.items()}
    for n in GROUP_SIZES:
        p = tmp_path / f"many{n}.hdf5"
        files[f"many{n}"] = (p, None)
        expect[f"many{n}"] = write_many(p, n)
    script = tmp_path / "read_with_h5py.py"
    script.write_text(_H5PY_SCRIPT)
    argv = [H5PY_PYTHON, str(script), str(tmp_path / "h5py_read.npz")]
    for tag, (p, _) in files.items():
        argv += [tag, str(p)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    done = subprocess.run(argv, capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stdout + done.stderr
    print(done.stdout.strip())
    got = np.load(tmp_path / "h5py_read.npz")
    for tag, (p, _) in files.items():
        read = {k.split(":d:", 1)[1]: got[k] for k in got.files if k.startswith(tag + ":d:")}
        assert sorted(read) == sorted(expect[tag])                    # h5py visited every object the writer was given
        for k, a in expect[tag].items():
            assert str(got[tag + ":t:" + k]) == a.dtype.str, k        # the type h5py sees, byte order included
            # (h5py hands a scalar back in native byte order; the swap back is exact)
            assert read[k].shape == a.shape and read[k].dtype.newbyteorder("=") == a.dtype.newbyteorder("="), k
            assert read[k].astype(a.dtype).tobytes() == a.tobytes(), k
        # keys() order: this project's reader on this writer's file against h5py on the same file
        mine, groups = _check(p, expect[tag])
        for gpath, keys in groups:
            assert list(got[tag + ":k:" + gpath]) == keys, gpath
        # and the same content from the file h5py wrote the reference's way
        theirs, their_groups = _check(str(p) + ".h5py", expect[tag])
        assert their_groups == groups
        for k in mine:
            assert mine[k].dtype == theirs[k].dtype and mine[k].tobytes() == theirs[k].tobytes(), k
