"""Write-only HDF5 containers in numpy: the surface step 3 of the data generation uses of h5py (``h5py.File(path, "w")``,
``create_group``, ``grp[name] = ndarray``, ``close``; synthetic-data-generation/step3_generate_h5_w_segs.py:28-51), producing the file
format h5py's defaults produce and ``io/hdf5.py`` reads: a version-0 superblock (8-byte offsets and lengths, group leaf K = 4, internal
K = 16), version-1 object headers, groups as a symbol-table message over a B-tree v1 and a local heap, contiguous datasets (dataspace
v1, datatype, fill value v2, layout v3 class 1), no modification times.  ``tests/golden/two_view_train_data.hdf5`` is the worked
example of every structure; the public "HDF5 File Format Specification Version 3.0" is the reference.

    with H5Writer(path) as f:
        grp = f.create_group("000000")
        grp["img"] = views                    # written to the file now
        grp["seg"] = labels

Raw data goes to the file as each dataset is assigned, so a container never sits in memory; only names, shapes and addresses are
kept.  The group metadata is built bottom-up and written by ``close()``, the superblock last: closing without an exception is the
only way to a valid file, and an exception inside the ``with`` block removes the partial file.  ``io.hdf5.H5File`` stays read-only.

Element types: integers and IEEE floats of either byte order (what ``io.hdf5._dtype_of`` accepts); anything else raises
``NotImplementedError`` naming the type.  No attributes, chunking, filters, links or resizing."""
from __future__ import annotations

import os
from typing import Dict, List, Tuple, Union

import numpy as np

_SIG = b"\x89HDF\r\n\x1a\n"
_UNDEF = 0xFFFFFFFFFFFFFFFF
_LEAF_K, _INTERNAL_K = 4, 16
_SNOD_ENTRIES, _TREE_CHILDREN = 2 * _LEAF_K, 2 * _INTERNAL_K
_SNOD_BYTES = 8 + _SNOD_ENTRIES * 40                          # 328
_TREE_BYTES = 24 + (2 * _TREE_CHILDREN + 1) * 8               # 544
_SUPERBLOCK_BYTES = 96
_HEAP_FREE_NULL = 1                                           # the library's end-of-free-list mark on disk


def _u(v: int, n: int) -> bytes:
    return int(v).to_bytes(n, "little")


def _pad8(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 8)


def _message(mtype: int, body: bytes, flags: int = 0) -> bytes:
    body = _pad8(body)
    return _u(mtype, 2) + _u(len(body), 2) + _u(flags, 1) + b"\0\0\0" + body


def _object_header(messages: List[bytes]) -> bytes:
    data = b"".join(messages)
    return b"\x01\x00" + _u(len(messages), 2) + _u(1, 4) + _u(len(data), 4) + b"\0\0\0\0" + data


def _datatype_message(dt: np.dtype) -> bytes:
    """Spec IV.A.2.d, version 1: fixed-point (class 0) or IEEE floating-point (class 1)."""
    big = 1 if dt.byteorder == ">" or (dt.byteorder == "=" and not np.little_endian) else 0
    size, bits = dt.itemsize, dt.itemsize * 8
    if dt.kind in "iu" and size in (1, 2, 4, 8):
        return bytes([0x10, big | (0x08 if dt.kind == "i" else 0), 0, 0]) + _u(size, 4) + _u(0, 2) + _u(bits, 2)
    if dt.kind == "f" and size in (2, 4, 8):
        exp_bits, man_bits = {2: (5, 10), 4: (8, 23), 8: (11, 52)}[size]
        return (bytes([0x11, big | 0x20, bits - 1, 0]) + _u(size, 4) + _u(0, 2) + _u(bits, 2)
                + bytes([man_bits, exp_bits, 0, man_bits]) + _u((1 << (exp_bits - 1)) - 1, 4))
    raise NotImplementedError(f"HDF5 datasets of dtype {dt} (only integers and IEEE floats of 1 to 8 bytes are written)")


def _dataset_header(shape: Tuple[int, ...], dt: np.dtype, addr: int, nbytes: int) -> bytes:
    rank = len(shape)
    dims = b"".join(_u(s, 8) for s in shape)
    space = bytes([1, rank, 1 if rank else 0, 0]) + b"\0\0\0\0" + dims + (dims if rank else b"")
    fill = bytes([2, 2, 2, 1]) + _u(0, 4)                     # version 2, late allocation, written if set, defined, size 0
    layout = bytes([3, 1]) + _u(addr, 8) + _u(nbytes, 8)      # version 3, contiguous
    return _object_header([_message(0x1, space), _message(0x3, _datatype_message(dt), 1), _message(0x5, fill, 1), _message(0x8, layout)])


class _Dataset:
    __slots__ = ("shape", "dtype", "addr", "nbytes")

    def __init__(self, shape, dtype, addr, nbytes):
        self.shape, self.dtype, self.addr, self.nbytes = shape, dtype, addr, nbytes


class H5WriteGroup:
    """A group of a file being written: ``create_group``, ``group[name] = ndarray``, ``group[name]`` for its subgroups."""

    def __init__(self, writer: "H5Writer", name: str):
        self._w, self.name = writer, name
        self._children: Dict[str, Union["H5WriteGroup", _Dataset]] = {}

    def _claim(self, name: str) -> str:
        self._w._require_open()
        if not isinstance(name, str):
            raise TypeError(f"link names are str (got {type(name).__name__})")
        if not name or "/" in name or name == "." or "\0" in name:
            raise ValueError(f"link name {name!r}: one non-empty path component")
        if name in self._children:
            raise ValueError(f"Unable to create link (name {name!r} already exists in {self.name!r})")
        return name

    def create_group(self, name: str) -> "H5WriteGroup":
        node = self
        parts = [p for p in name.split("/") if p] if isinstance(name, str) else [name]
        if not parts:
            raise ValueError(f"group name {name!r} is empty")
        for part in parts[:-1]:                                # intermediate groups, as h5py creates them
            nxt = node._children.get(part)
            node = nxt if isinstance(nxt, H5WriteGroup) else node.create_group(part)
        grp = H5WriteGroup(node._w, node.name.rstrip("/") + "/" + parts[-1])
        node._children[node._claim(parts[-1])] = grp
        return grp

    def __setitem__(self, name: str, value):
        name = self._claim(name)
        arr = np.asarray(value)
        _datatype_message(arr.dtype)                           # refuses before anything is written
        if not arr.flags.c_contiguous:                         # (np.ascontiguousarray would make a zero-dimensional array 1-D)
            arr = np.ascontiguousarray(arr)
        addr = self._w._append(arr.tobytes() if arr.ndim == 0 else arr.reshape(-1).view(np.uint8).data) if arr.size else _UNDEF
        self._children[name] = _Dataset(tuple(int(s) for s in arr.shape), arr.dtype, addr, arr.nbytes)

    def __getitem__(self, name: str) -> "H5WriteGroup":
        node = self
        for part in [p for p in name.split("/") if p]:
            node = node._children.get(part) if isinstance(node, H5WriteGroup) else None
            if not isinstance(node, H5WriteGroup):
                raise KeyError(f"{name!r}: no such group (datasets of a file being written cannot be read back)")
        return node

    def __contains__(self, name):
        return name in self._children

    def __len__(self):
        return len(self._children)

    def keys(self):
        return sorted(self._children, key=lambda s: s.encode("utf-8"))

    # ---- metadata, bottom-up -----------------------------------------------------------------------------------------------------
    def _emit(self) -> Tuple[int, int, int]:
        """Writes everything below this group, then its heap, symbol-table nodes, B-tree and header -> their addresses
        (header, B-tree root, heap)."""
        w = self._w
        names = self.keys()
        heap = bytearray(8)                                    # offset 0: the empty string, key 0 of the leftmost B-tree node
        entries = []
        for name in names:
            child = self._children[name]
            off = len(heap)
            heap += _pad8(name.encode("utf-8") + b"\0")
            if isinstance(child, H5WriteGroup):
                hdr, tree, hp = child._emit()
                entries.append((off, _u(off, 8) + _u(hdr, 8) + _u(1, 4) + _u(0, 4) + _u(tree, 8) + _u(hp, 8)))
            else:
                hdr = w._append(_dataset_header(child.shape, child.dtype, child.addr, child.nbytes))
                entries.append((off, _u(off, 8) + _u(hdr, 8) + _u(0, 4) + _u(0, 4) + bytes(16)))
        free_at = len(heap)
        heap += _u(_HEAP_FREE_NULL, 8) + _u(16, 8)             # one free block at the end: next, size
        heap_addr = w._align()
        w._append(b"HEAP\0\0\0\0" + _u(len(heap), 8) + _u(free_at, 8) + _u(heap_addr + 32, 8) + bytes(heap))

        # symbol-table nodes of up to 8 entries in name order: (address, heap offset of the largest name)
        level: List[Tuple[int, int]] = []
        for i in range(0, len(entries), _SNOD_ENTRIES):
            chunk = entries[i:i + _SNOD_ENTRIES]
            node = b"SNOD\x01\0" + _u(len(chunk), 2) + b"".join(e for _, e in chunk)
            level.append((w._append(node.ljust(_SNOD_BYTES, b"\0")), chunk[-1][0]))

        # B-tree v1 nodes of up to 32 children, level by level until one root is left (an empty group: one empty leaf node)
        depth = 0
        while True:
            groups = [level[i:i + _TREE_CHILDREN] for i in range(0, len(level), _TREE_CHILDREN)] or [[]]
            base = w._align()
            nxt = []
            left_key = 0
            for i, kids in enumerate(groups):
                left = base + (i - 1) * _TREE_BYTES if i else _UNDEF
                right = base + (i + 1) * _TREE_BYTES if i + 1 < len(groups) else _UNDEF
                node = b"TREE\0" + _u(depth, 1) + _u(len(kids), 2) + _u(left, 8) + _u(right, 8) + _u(left_key, 8)
                for addr, key in kids:
                    node += _u(addr, 8) + _u(key, 8)
                    left_key = key
                nxt.append((w._append(node.ljust(_TREE_BYTES, b"\0")), left_key))
            level, depth = nxt, depth + 1
            if len(level) == 1:
                break
        tree_addr = level[0][0]
        hdr = w._append(_object_header([_message(0x11, _u(tree_addr, 8) + _u(heap_addr, 8))]))
        return hdr, tree_addr, heap_addr


class H5Writer(H5WriteGroup):
    """The file being written; its own root group.  A context manager: leaving the block normally closes the file, leaving it
    through an exception removes it."""

    def __init__(self, path):
        self.filename = os.fspath(path)
        self._fh = open(self.filename, "wb")
        self._fh.write(bytes(_SUPERBLOCK_BYTES))               # the superblock is written last
        self._pos = _SUPERBLOCK_BYTES
        super().__init__(self, "/")

    def _require_open(self):
        if self._fh is None:
            raise ValueError(f"{self.filename}: the file is closed")

    def _align(self) -> int:
        pad = -self._pos % 8
        if pad:
            self._fh.write(bytes(pad))
            self._pos += pad
        return self._pos

    def _append(self, data) -> int:
        addr = self._align()
        self._fh.write(data)
        self._pos += len(data)
        return addr

    def close(self):
        if self._fh is None:
            return
        try:
            hdr, tree, heap = self._emit()
            eof = self._align()
            root = _u(0, 8) + _u(hdr, 8) + _u(1, 4) + _u(0, 4) + _u(tree, 8) + _u(heap, 8)
            sb = (_SIG + bytes([0, 0, 0, 0, 0, 8, 8, 0]) + _u(_LEAF_K, 2) + _u(_INTERNAL_K, 2) + _u(0, 4)
                  + _u(0, 8) + _u(_UNDEF, 8) + _u(eof, 8) + _u(_UNDEF, 8) + root)
            assert len(sb) == _SUPERBLOCK_BYTES
            self._fh.seek(0)
            self._fh.write(sb)
            self._fh.close()
            self._fh = None
        except BaseException:
            self.discard()
            raise

    def discard(self):
        """Closes and removes the partial file."""
        if self._fh is not None:
            self._fh.close()
            self._fh = None
            if os.path.exists(self.filename):
                os.remove(self.filename)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.discard()
        return False
