"""Constants of a TensorFlow frozen graph (`.pb`, a serialised GraphDef) without TensorFlow.

The reference converts `ssd_mobilenet_v1_coco.pb` through graphsurgeon + UFF (fastmot/models/ssd.py:52-96); here the
protobuf wire format is read directly with the primitives of models/onnx_reader.py.  Only what a weight source needs:

    GraphDef    node = 1
    NodeDef     name = 1, op = 2, attr = 5 (map entry: key = 1, value = 2)
    AttrValue   tensor = 8
    TensorProto dtype = 1 (DT_FLOAT = 1, DT_INT32 = 3), tensor_shape = 2 (TensorShapeProto: dim = 2 -> size = 1),
                tensor_content = 4, float_val = 5, int_val = 7

`read_constants` returns {node name: ndarray} for every `Const` node; a single repeated value is broadcast over the
shape (TensorFlow stores constant-filled tensors that way).  Anything else is skipped.  Neither TensorFlow nor a frozen
graph exists where this was written: the field numbers are DERIVED from tensorflow/core/framework/*.proto as published,
not pinned against a file; tests/pb_writer.py writes the same fields independently.
"""
from pathlib import Path

import numpy as np

from .onnx_reader import _fields, _floats, _ints

DT_FLOAT, DT_INT32 = 1, 3
_DTYPES = {DT_FLOAT: np.float32, DT_INT32: np.int32}


def _messages(buf):
    """_fields with truncation reported as ValueError (a fixed-width field or a varint cut short)."""
    try:
        for f, wt, v in _fields(buf):
            if wt in (1, 5) and len(v) != (8 if wt == 1 else 4):
                raise ValueError('truncated frozen graph')
            yield f, wt, v
    except IndexError:
        raise ValueError('truncated frozen graph') from None


def _shape(buf):
    dims = []
    for f, _, v in _messages(buf):
        if f == 2:                                   # dim
            size = 0
            for f2, wt2, v2 in _messages(v):
                if f2 == 1:
                    size = _ints(wt2, v2)[0]
            dims.append(size)
    return dims


def _tensor(buf, name):
    dtype, dims, content, floats, ints = 0, [], None, [], []
    for f, wt, v in _messages(buf):
        if f == 1:
            dtype = v
        elif f == 2:
            dims = _shape(v)
        elif f == 4:
            content = v
        elif f == 5:
            if wt == 2 and len(v) % 4:
                raise ValueError('truncated frozen graph')
            floats.append(_floats(wt, v))
        elif f == 7:
            ints += _ints(wt, v)
    if dtype not in _DTYPES:
        return None                                  # strings, bools, ...: not weights
    dt = np.dtype(_DTYPES[dtype])
    if any(d < 0 for d in dims):
        raise ValueError(f'{name}: unknown dimension in a constant')
    n = int(np.prod(dims)) if dims else 1
    if content is not None and len(content):
        if len(content) != n * dt.itemsize:
            raise ValueError(f'{name}: {len(content)} bytes of tensor_content for shape {dims}')
        a = np.frombuffer(content, dt.newbyteorder('<'))
    else:
        a = np.concatenate(floats).astype(dt) if dtype == DT_FLOAT and floats else np.asarray(ints, dt)
        if a.size == 1 and n != 1:
            a = np.full(n, a[0], dt)
        elif a.size == 0 and n:                      # (an all-zero constant may carry no value at all)
            a = np.zeros(n, dt)
        elif a.size != n:
            raise ValueError(f'{name}: {a.size} values for shape {dims}')
    return np.array(a, dt).reshape(dims)


def _node(buf):
    name, op, tensor = '', '', None
    for f, _, v in _messages(buf):
        if f == 1:
            name = bytes(v).decode()
        elif f == 2:
            op = bytes(v).decode()
        elif f == 5:
            key, value = '', None
            for f2, _, v2 in _messages(v):
                if f2 == 1:
                    key = bytes(v2).decode()
                elif f2 == 2:
                    value = v2
            if key == 'value' and value is not None:
                for f3, _, v3 in _messages(value):
                    if f3 == 8:
                        tensor = v3
    return name, op, tensor


def read_constants(source):
    """source: path or bytes of a GraphDef -> {node name: ndarray} of its Const nodes (float32 / int32)."""
    data = Path(source).read_bytes() if isinstance(source, (str, Path)) else bytes(source)
    out = {}
    for f, wt, v in _messages(memoryview(data)):
        if f != 1 or wt != 2:
            continue
        name, op, tensor = _node(v)
        if op != 'Const' or tensor is None:
            continue
        a = _tensor(tensor, name)
        if a is not None:
            out[name] = a
    return out
