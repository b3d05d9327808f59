"""Writes tests/golden/cppn_ref.npz from the reference's own `cppn.py`:  python tools/make_cppn_golden.py /path/to/reference

The reference file cannot be imported whole (it imports clip, torchvision and eps at module level), so it is parsed with `ast` and only the
`ConvLayer`, `CPPN`, `get_mgrid` and `export_data` definitions are compiled, at run time; none of its text is copied anywhere.  Everything runs on
the CPU (CPPN.forward moves its input to the GPU, so the image is taken from `model.net` directly).

Per case k = (H, W, layers, nf, act):  c<k>_cfg, c<k>_seed, c<k>_params (every parameter after torch.manual_seed(seed); CPPN(...), flat in
state_dict order), c<k>_tail (the next three torch.rand values), c<k>_mgrid (get_mgrid, cast to f32), c<k>_img64 (the image with weights
and grid cast to fp64), c<k>_drgb and c<k>_grad64 (the fp64 gradient of sum(image * drgb), flat).  `keys` = the state_dict keys of the last
case; export_<i> = export_data's arrays for case 0."""
import ast
import math
import os
import sys
import tempfile
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ['unbias', 'comp', 'relu']
CASES = [(24, 40, 3, 8, 'unbias'), (40, 56, 10, 24, 'unbias'), (40, 56, 10, 24, 'comp'), (40, 56, 10, 24, 'relu')]
WANTED = ('ConvLayer', 'CPPN', 'get_mgrid', 'export_data')


def reference_namespace(ref_root):
    path = os.path.join(ref_root, 'cppn.py')
    tree = ast.parse(open(path).read(), path)
    nodes = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in WANTED]
    assert sorted(n.name for n in nodes) == sorted(WANTED), [n.name for n in nodes]
    ns = dict(torch=torch, nn=nn, F=F, np=np, math=math, OrderedDict=OrderedDict)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return ns


def main(ref_root):
    ns = reference_namespace(ref_root)
    out = {}
    for k, (h, w, layers, nf, act) in enumerate(CASES):
        seed = 100 + k
        torch.manual_seed(seed)
        model = ns['CPPN'](2, nf, layers, 3, act_fn=act)
        tail = torch.rand(3)
        sd = model.state_dict()
        mgrid = ns['get_mgrid'](h, w).astype(np.float32)                 # cppn.py:175-176 with a.size = [H, W]
        assert mgrid.shape == (1, 2, h, w) and mgrid[0, 0, 0, -1] == 1 and mgrid[0, 0, -1, 0] == -1       # channel 0 = x along W
        net64 = ns['CPPN'](2, nf, layers, 3, act_fn=act).double()
        net64.load_state_dict(OrderedDict((key, v.double()) for key, v in sd.items()))
        drgb = torch.randn(3, h, w, generator=torch.Generator().manual_seed(seed + 1000)) / (h * w)
        img = net64.net(torch.from_numpy(mgrid).double())
        (img[0] * drgb.double()).sum().backward()
        pre = 'c%d_' % k
        out[pre + 'cfg'] = np.array([h, w, layers, nf, ACTS.index(act)], dtype=np.int64)
        out[pre + 'seed'] = np.array(seed, dtype=np.int64)
        out[pre + 'params'] = torch.cat([v.reshape(-1) for v in sd.values()]).numpy()
        out[pre + 'tail'] = tail.numpy()
        out[pre + 'mgrid'] = mgrid
        out[pre + 'img64'] = img.detach()[0].numpy()
        out[pre + 'drgb'] = drgb.numpy()
        out[pre + 'grad64'] = torch.cat([p.grad.reshape(-1) for p in net64.parameters()]).numpy()
        if k == 0:
            with tempfile.TemporaryDirectory() as d:
                ns['export_data'](sd, os.path.join(d, 'snap'), [h, w])
                arrays = np.load(os.path.join(d, 'snap.npy'), allow_pickle=True)
            out['export_n'] = np.array(len(arrays), dtype=np.int64)
            for i, a in enumerate(arrays):
                out['export_%d' % i] = np.asarray(a)
        out['keys'] = np.array(list(sd.keys()))
    path = os.path.join(ROOT, 'tests', 'golden', 'cppn_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
