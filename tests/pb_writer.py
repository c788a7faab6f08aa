"""TEST INFRASTRUCTURE: a minimal TensorFlow GraphDef writer (protobuf wire format by hand, no tensorflow package),
the counterpart of tests/onnx_writer.py for models/tf_graph_reader.py.  Written from tensorflow/core/framework
graph.proto / node_def.proto / attr_value.proto / tensor.proto / tensor_shape.proto, independently of the reader."""
import struct

import numpy as np

DT_FLOAT, DT_INT32, DT_STRING = 1, 3, 7


def varint(n):
    n &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = n & 0x7f
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def field(num, payload):
    """length-delimited field"""
    return varint(num << 3 | 2) + varint(len(payload)) + payload


def vfield(num, value):
    return varint(num << 3) + varint(value)


def shape(dims):
    return b''.join(field(2, vfield(1, d)) for d in dims)


def tensor(array, form='content', dims=None):
    """form: 'content' (tensor_content bytes), 'float_val' / 'int_val' (packed repeated values), 'scalar' (ONE value, to
    be broadcast over `dims`)."""
    a = np.asarray(array)
    dt = DT_FLOAT if a.dtype.kind == 'f' else DT_INT32
    dims = list(a.shape) if dims is None else list(dims)
    body = vfield(1, dt) + field(2, shape(dims))
    flat = a.reshape(-1)
    if form == 'content':
        body += field(4, flat.astype('<f4' if dt == DT_FLOAT else '<i4').tobytes())
    elif dt == DT_FLOAT:
        vals = flat[:1] if form == 'scalar' else flat
        body += field(5, vals.astype('<f4').tobytes())
    else:
        vals = flat[:1] if form == 'scalar' else flat
        body += field(7, b''.join(varint(int(v)) for v in vals))
    return body


def attr(key, value_bytes):
    return field(5, field(1, key.encode()) + field(2, value_bytes))


def const_node(name, array, form='content', dims=None):
    a = np.asarray(array)
    dt = DT_FLOAT if a.dtype.kind == 'f' else DT_INT32
    return field(1, name.encode()) + field(2, b'Const') + attr('dtype', vfield(6, dt)) + \
        attr('value', field(8, tensor(a, form, dims)))


def op_node(name, op, inputs=()):
    return field(1, name.encode()) + field(2, op.encode()) + b''.join(field(3, i.encode()) for i in inputs) + \
        attr('T', vfield(6, DT_FLOAT))


def graph_def(nodes):
    return b''.join(field(1, n) for n in nodes) + field(4, vfield(1, 27))       # + versions { producer: 27 }


def frozen_graph(arrays):
    """{variable name: array} -> GraphDef bytes: one Const per variable and, as freeze_graph leaves them, an Identity
    `<name>/read` behind each."""
    nodes = []
    for name, a in arrays.items():
        nodes.append(const_node(name, np.asarray(a, np.float32)))
        nodes.append(op_node(name + '/read', 'Identity', [name]))
    return graph_def(nodes)
