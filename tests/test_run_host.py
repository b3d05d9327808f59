"""aphantasia_amd/run.py: the host code clip_fft.py, illustrip.py and cppn.py share (no GPU: nothing here creates a model or an engine)"""
import ast
import os
import pickle
import sys

import pytest
import torch

from aphantasia_amd import comm, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_ENV = ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'APH_RUN_ID', 'HSA_ENABLE_IPC_MODE_LEGACY')


def test_split_prompt_is_upstreams_rule():
    """clip_fft.py:145-149 == illustrip.py:186-190 upstream: split at '|', an optional ':weight', nothing stripped from the text"""
    assert run.split_prompt('a') == [('a', 1.0)]
    assert run.split_prompt('a|b') == [('a', 1.0), ('b', 1.0)]
    assert run.split_prompt('a:0.5|b') == [('a', 0.5), ('b', 1.0)]
    assert run.split_prompt(' a : 2 ') == [(' a ', 2.0)]
    with pytest.raises(ValueError):
        run.split_prompt('a:1:2')


def test_dual_step_is_the_slice():
    for steps in range(1, 41):
        for dm in range(1, 8):
            assert [i for i in range(steps) if run.is_dual_step(i, dm)] == list(range(steps))[dm::dm]
        assert not any(run.is_dual_step(i, None) for i in range(steps))


class _Eng:
    calls = 0

    def global_loss(self):
        self.calls += 1
        return 0.25


def test_progress_cadence_and_lines(capsys):
    for n in range(1, 26):
        eng, prog = _Eng(), run.Progress(n, 'step', True)
        want = [i for i in range(n) if i % 10 == 9 or i == n - 1]
        assert [i for i in range(n) if prog.due(i)] == want
        for i in range(n):
            prog.tick(i, eng)
        lines = capsys.readouterr().out.splitlines()
        assert eng.calls == len(want) == len(lines)
        for i, line in zip(want, lines):
            assert line.startswith(' step %d/%d  loss 0.2500  ' % (i + 1, n)) and line.endswith(' steps/s')
    # a quiet rank of a multi-rank run still takes part in the collective and prints nothing; a quiet single rank does neither
    for world, calls in ((2, 2), (1, 0)):
        eng, prog = _Eng(), run.Progress(12, 'frame', False, world)
        for i in range(12):
            prog.tick(i, eng)
        assert eng.calls == calls and capsys.readouterr().out == ''
    prog = run.Progress(12, 'frame', True, 2)
    prog.tick(11, _Eng())
    prog.done()
    tick, done = capsys.readouterr().out.splitlines()
    assert tick.startswith(' frame 12/12  loss 0.2500  ') and tick.endswith(' frames/s')
    assert done.startswith(' done: 12 frames in ') and done.endswith(' frames/s) on 2 ranks')
    run.Progress(3, 'step', False).done()
    done = capsys.readouterr().out
    assert done.startswith(' done: 3 steps in ') and done.endswith(' steps/s)\n')


def _stub_main(argv):
    _stub_main.seen = (list(argv), {k: os.environ.get(k) for k in RANK_ENV})


@pytest.mark.parametrize('script, prefix', [('clip_fft', 'r'), ('illustrip', 'i')])
def test_spawn_branch(monkeypatch, script, prefix):
    """--ranks N outside torchrun: the children get the parent's argv (plus a drawn --seed when there is none), a port in 20000..39999 and
    a run id of the program's letter and the parent's pid; what is handed to torch.multiprocessing.spawn pickles"""
    mod = __import__(script)
    rec = []
    monkeypatch.setattr(comm, 'spawn_ranks', lambda fn, args, nranks: rec.append((fn, args, nranks)))
    monkeypatch.delenv('RANK', raising=False)
    argv = ['-t', 'cat', '--ranks', '2']
    assert mod.main(list(argv)) is None
    assert mod.main(argv + ['--seed', '5']) is None
    (fn, args, nranks), (fn5, args5, _) = rec
    main, child_argv, world, port, run_id = args
    assert fn is fn5 is run._rank_entry and main is mod.main and nranks == world == 2
    assert child_argv[:4] == argv and child_argv[4] == '--seed' and 0 <= int(child_argv[5]) < 2 ** 24 and len(child_argv) == 6
    assert 20000 <= port < 40000 and run_id == '%s%d' % (prefix, os.getpid())
    assert args5[1] == argv + ['--seed', '5']
    pickle.dumps((fn, args))


def test_rank_entry_sets_the_rank_environment(monkeypatch):
    """the child entry of a spawned rank: exactly these seven variables, then the program's main on the parent's argv"""
    for k in RANK_ENV:
        monkeypatch.delenv(k, raising=False)
    before = dict(os.environ)
    try:
        run._rank_entry(1, _stub_main, ['-t', 'x'], 2, 23456, 'r77')
        argv, env = _stub_main.seen
        assert argv == ['-t', 'x']
        assert env == dict(RANK='1', LOCAL_RANK='1', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT='23456', APH_RUN_ID='r77',
                           HSA_ENABLE_IPC_MODE_LEGACY='0')
        assert {k for k in os.environ if os.environ[k] != before.get(k)} == set(RANK_ENV)
    finally:
        os.environ.clear()
        os.environ.update(before)


@pytest.mark.parametrize('script', ['clip_fft', 'illustrip'])
def test_multi_rank_needs_a_seed(monkeypatch, script):
    """under torchrun (WORLD_SIZE > 1) an unseeded run is refused before any process group or device is touched"""
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setattr(comm, 'create', lambda *a, **k: pytest.fail('no communicator before the seed check'))
    with pytest.raises(SystemExit, match=r'^ multi-rank runs need --seed \(every rank draws the same crop / augment tables and takes its share of the cuts\)$'):
        __import__(script).main(['-t', 'cat'])


def test_quiet_fields_are_set_on_non_zero_ranks_only(monkeypatch):
    import argparse
    monkeypatch.setattr(comm, 'create', lambda rank, world: 'comm%d' % rank)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setenv('WORLD_SIZE', '2')
    for rank in (0, 1):
        monkeypatch.setenv('RANK', str(rank))
        a = argparse.Namespace(ranks=1, seed=3, verbose=True, no_save=False, depth_dir='d')
        assert run.bootstrap_ranks(a, None, _stub_main, 'i', verbose=False, no_save=True, depth_dir=None) == (rank, 2, 'comm%d' % rank)
        assert (a.verbose, a.no_save, a.depth_dir) == ((True, False, 'd') if rank == 0 else (False, True, None))


def test_load_aest(tmp_path):
    assert run.load_aest(None, 0) is None and run.load_aest(str(tmp_path / 'missing.pth'), 0) is None
    for path in (None, str(tmp_path / 'missing.pth')):
        with pytest.raises(SystemExit, match='--aest needs the LAION linear head'):
            run.load_aest(path, 0.5)
    path = str(tmp_path / 'head.pth')
    weight = torch.arange(8, dtype=torch.float64).reshape(1, 8)
    torch.save({'weight': weight, 'bias': torch.tensor([0.75])}, path)
    w, b, s = run.load_aest(path, 0.5)
    assert w.dtype == torch.float32 and torch.equal(w, weight.float()) and (b, s) == (0.75, 0.5)

    class Model:
        name = 'ViT-B/32'
        class visual: output_dim = 8
    run.check_aest(None, Model, '--aest-weights')
    run.check_aest((w, b, s), Model, '--aest-weights')
    Model.visual.output_dim = 16
    with pytest.raises(SystemExit, match='--aest-weights2: a head of 8 inputs, but ViT-B/32 encodes into 16'):
        run.check_aest((w, b, s), Model, '--aest-weights2')


def test_seed_all():
    import numpy as np
    run.seed_all(7)
    t, n = torch.rand(3), np.random.rand(3)
    run.seed_all(None)                       # no seed: the generators are left alone
    run.seed_all(7)
    assert torch.equal(torch.rand(3), t) and (np.random.rand(3) == n).all()


def test_illustrip_and_cppn_do_not_load_the_clip_fft_script(monkeypatch):
    for name in ('clip_fft', 'illustrip', 'cppn'):
        monkeypatch.delitem(sys.modules, name, raising=False)
    import illustrip, cppn  # noqa: E401,F401
    assert 'clip_fft' not in sys.modules
    for name in ('illustrip.py', 'cppn.py'):              # ... and not from inside a function either
        for node in ast.walk(ast.parse(open(os.path.join(ROOT, name)).read())):
            names = [n.name for n in node.names] if isinstance(node, ast.Import) else [node.module] if isinstance(node, ast.ImportFrom) else []
            assert 'clip_fft' not in names


def test_clip_fft_re_exports():
    import clip_fft
    assert clip_fft.FrameWriter is run.FrameWriter and clip_fft.FrameWriter.THREADS == 4 and clip_fft.FrameWriter.RING == 16
    assert clip_fft.check_samples is run.check_samples and clip_fft.pick_transform is run.pick_transform
