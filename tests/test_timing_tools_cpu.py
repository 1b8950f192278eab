"""The measuring protocol of the tools/time_*.py scripts (tools/timing.py), without a GPU.

Replay: the recorded files under profiles/ hold the children's raw lines (those with `process`) followed by the summaries of
the same invocation.  Each ported script's parent path is fed the raw lines back -- subprocess.run, the one place a child is
started, is replaced by a fake that returns the recorded stdout of process p -- and has to emit the recorded summaries, floats
and key order exactly.  CPE_TIMING_TOOLS names another copy of the scripts to replay against (one that predates timing.py
passes the replay unchanged; the tests of timing.py itself then do not apply).

Parent rule: a throw-away child script shows that the children run strictly one after the other and that the first one that
fails or outlives its limit is the last one started."""
import argparse
import glob
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.environ.get('CPE_TIMING_TOOLS', os.path.join(ROOT, 'tools'))
SCRIPTS = ('time_prestep', 'time_multiframe', 'time_frame_angles', 'time_match_offset', 'time_plane_fit', 'time_table_tri',
           'time_projector_model', 'time_index_shift', 'time_multiframe_consensus', 'time_fused_tri', 'time_relabel', 'time_grid_refine')
NO_LM = 'r11_time_multiframe'            # predates the lm variants: the summary code of its script raises KeyError('lm') on it


def _values(rows, kind, field):
    """the distinct values of a field over process 0's rows of a kind, in order, as command-line words"""
    out = []
    for d in rows:
        if d['process'] == 0 and d['kind'] == kind and str(round(d[field])) not in out:
            out.append(str(round(d[field])))
    return out


ARGS = dict(                             # script -> its own arguments, from the rows of one invocation
    time_prestep=lambda r: ['--pairs'] + _values(r, 'case', 'pairs'),
    time_multiframe=lambda r: ['--frames'] + _values(r, 'case', 'frames') + ['--points'] + _values(r, 'case', 'points'),
    time_frame_angles=lambda r: ['--frames'] + _values(r, 'case', 'frames') + ['--points'] + _values(r, 'case', 'points'),
    time_match_offset=lambda r: ['--frames'] + _values(r, 'case', 'frames') + ['--points'] + _values(r, 'case', 'points'),
    time_plane_fit=lambda r: ['--frames'] + _values(r, 'fit', 'frames') + ['--table-frames'] + _values(r, 'table', 'frames'),
    time_table_tri=lambda r: (['--frames'] + _values(r, 'tables', 'frames') +
                              ['--pipeline-frames'] + (_values(r, 'pipeline', 'frames') or ['0']) + ['--chunk'] + (_values(r, 'pipeline', 'chunk') or ['32'])),
    time_projector_model=lambda r: ['--frames'] + _values(r, 'projector', 'frames'),
    time_index_shift=lambda r: ['--frames'] + _values(r, 'tables', 'frames') + ['--fit-frames'] + (_values(r, 'fit', 'frames') or ['0']),
    time_multiframe_consensus=lambda r: (['--frames'] + _values(r, 'case', 'frames') + ['--points'] + _values(r, 'case', 'points') +
                                         ['--bad'] + _values(r, 'case', 'bad')),
    time_fused_tri=lambda r: ['--frames'] + _values(r, 'tables', 'frames'),
    time_relabel=lambda r: ['--frames'] + _values(r, 'relabel', 'frames'),
    # the count of --points values is the number of rows per frame size and process
    time_grid_refine=lambda r: ['--frames'] + _values(r, 'tables', 'frames') + ['--points'] + [
        str(round(d['points'])) for d in r if d['process'] == 0 and d['frames'] == r[0]['frames']],
)


def _invocations():
    """-> [(id, script, raw rows, summaries)] of every recorded invocation of the twelve scripts; a file that holds two is
    split at the first raw line that follows a summary line"""
    out, without_summary = [], set()
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_time_*.jsonl'))):
        name = os.path.basename(path)[:-len('.jsonl')]
        stem = re.sub(r'^r\d+_', '', name)
        script = max((s for s in SCRIPTS if stem.startswith(s)), key=len, default=None)
        if script is None or name == NO_LM:
            continue
        parts = []
        with open(path) as f:
            for d in (json.loads(ln) for ln in f if ln.startswith('{')):
                raw = 'process' in d
                if raw and (not parts or parts[-1][1]):
                    parts.append(([], []))
                parts[-1][0 if raw else 1].append(d)
        for i, (rows, summaries) in enumerate(parts):
            if summaries:
                out.append((f'{name}[{i}]', script, rows, summaries))
            else:
                without_summary.add(name)
    assert without_summary <= {'r25_time_grid_refine_new', 'r25_time_grid_refine_parent'}, without_summary
    return out


INVOCATIONS = _invocations()


def _load(script, monkeypatch):
    monkeypatch.setattr(sys, 'path', [TOOLS] + sys.path)     # a copy: what the scripts put on sys.path goes with the test
    spec = importlib.util.spec_from_file_location('replayed_' + script, os.path.join(TOOLS, script + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_script_has_a_recorded_invocation():
    assert {script for _, script, _, _ in INVOCATIONS} == set(SCRIPTS)


@pytest.mark.parametrize('name,script,rows,summaries', INVOCATIONS, ids=[i[0] for i in INVOCATIONS])
def test_replay_reproduces_the_recorded_summaries(name, script, rows, summaries, monkeypatch, capsys, tmp_path):
    procs = max(d['process'] for d in rows) + 1
    started = []

    def fake_run(cmd, stdout=None, text=None, check=None, timeout=None):
        assert '--child' in cmd and check and timeout > 0
        p = len(started)
        started.append(cmd)
        mine = [{k: v for k, v in d.items() if k != 'process'} for d in rows if d['process'] == p]
        return subprocess.CompletedProcess(cmd, 0, stdout='warming up\n' + ''.join(json.dumps(d) + '\n' for d in mine))
    mod = _load(script, monkeypatch)
    out = tmp_path / 'out.jsonl'
    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.setattr(sys, 'argv', [script + '.py', '--procs', str(procs), '--out', str(out)] + ARGS[script](rows))
    assert mod.main() == 0
    printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()]
    assert len(started) == procs
    assert printed == rows + summaries                                           # parsed JSON, floats exactly
    assert [list(d) for d in printed] == [list(d) for d in rows + summaries]     # and the key order of every line
    assert [json.loads(ln) for ln in out.read_text().splitlines()] == printed


# ---- the parent rule, on a throw-away child

CHILD = '''import json, sys, time
marker, mode = sys.argv[sys.argv.index('--marker') + 1:][:2]
assert sys.argv[1] == '--child'
with open(marker, 'a+') as f:
    f.seek(0)
    p = len(f.read().split())
    f.write(f'{p} ')
print('not a line of the protocol')
print(json.dumps(dict(kind='case', frames=45, reps=2, median_ms=dict(a=1.0 + p, b=5.0 - p), ms=dict(a=[1.0], b=[5.0]), status_ok=45)))
print(json.dumps(dict(kind='other', n=p)), flush=True)
if p == 1 and mode == 'fail':
    sys.exit(3)
if p == 1 and mode == 'hang':
    time.sleep(60)
'''


@pytest.fixture
def timing(monkeypatch):
    if not os.path.exists(os.path.join(TOOLS, 'timing.py')):
        pytest.skip('the scripts replayed predate tools/timing.py')
    return _load('timing', monkeypatch)


def _parent(timing, tmp_path, mode, child_timeout):
    """what a script's main() does after parsing: the children, then one summary"""
    script = tmp_path / 'child.py'
    script.write_text(CHILD)
    a = argparse.Namespace(procs=3, child_timeout=child_timeout, out=str(tmp_path / 'out.jsonl'))
    rows, emit = timing.run_children(str(script), a, ['--marker', str(tmp_path / 'marker'), mode])
    emit(dict(kind='summary', n=len(rows)))
    return rows


def test_children_run_in_order_and_every_line_is_tagged_printed_and_appended(timing, tmp_path, capsys):
    rows = _parent(timing, tmp_path, 'ok', 30.0)
    assert (tmp_path / 'marker').read_text().split() == ['0', '1', '2']
    assert [(d['kind'], d.get('process')) for d in rows] == [('case', 0), ('other', 0), ('case', 1), ('other', 1), ('case', 2), ('other', 2),
                                                             ('summary', None)]
    assert all(list(d)[-1] == 'process' for d in rows[:-1]) and [d['n'] for d in rows[1:-1:2]] == [0, 1, 2]
    printed = capsys.readouterr().out.splitlines()
    assert all(ln.startswith('{') for ln in printed) and [json.loads(ln) for ln in printed] == rows
    assert [json.loads(ln) for ln in (tmp_path / 'out.jsonl').read_text().splitlines()] == rows


@pytest.mark.parametrize('mode,child_timeout,error', [('fail', 30.0, subprocess.CalledProcessError), ('hang', 0.9, subprocess.TimeoutExpired)])
def test_the_first_child_that_fails_or_outlives_its_limit_is_the_last_one_started(timing, tmp_path, capsys, mode, child_timeout, error):
    with pytest.raises(error):
        _parent(timing, tmp_path, mode, child_timeout)
    assert (tmp_path / 'marker').read_text().split() == ['0', '1']               # the third never started
    emitted = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()]
    assert [(d['kind'], d['process']) for d in emitted] == [('case', 0), ('other', 0)]   # no line of the failed child, no summary
    assert [json.loads(ln) for ln in (tmp_path / 'out.jsonl').read_text().splitlines()] == emitted


def test_reduction_across_children(timing):
    def row(p, a, b, ev):
        return dict(kind='case', frames=45, reps=7, median_ms=dict(a=a, b=b), median_event_ms=dict(a=ev), status_ok=45 - p, note=[p], ms=dict(a=[a]),
                    process=p)
    odd = [row(0, 3.0, 10.0, 0.5), row(1, 1.0, 14.0, 0.25), row(2, 2.5, 11.0, 1.0)]
    assert timing.reduce(odd) == (dict(a=2.5, b=11.0), dict(a=2.0, b=4.0))
    assert timing.reduce(odd + [row(3, 2.0, 12.0, 0.75)]) == (dict(a=2.25, b=11.5), dict(a=2.0, b=4.0))   # even: mean of the middle two
    assert timing.reduce(odd, ('b',)) == (dict(b=11.0), dict(b=4.0))
    assert timing.reduce(odd, field='median_event_ms') == (dict(a=0.5), dict(a=0.75))
    # everything the summary does not have yet comes from process 0's row, in that row's order, without reps, ms and process
    carried = timing.carry(dict(kind='summary', frames=45, procs=3), odd)
    assert carried == dict(kind='summary', frames=45, procs=3, median_ms=dict(a=3.0, b=10.0), median_event_ms=dict(a=0.5), status_ok=45, note=[0])
    assert list(carried) == ['kind', 'frames', 'procs', 'median_ms', 'median_event_ms', 'status_ok', 'note']
    assert 'note' not in timing.carry(dict(kind='summary'), odd, skip=('note',))
    s = timing.ratio_summary(dict(kind='case_summary', frames=45, procs=3), odd, (('a_over_b', 'a', 'b'),))
    assert s == dict(kind='case_summary', frames=45, procs=3, median_ms=dict(a=2.5, b=11.0), spread_ms=dict(a=2.0, b=4.0), a_over_b=2.5 / 11.0,
                     median_event_ms=dict(a=0.5), status_ok=45, note=[0])
    assert list(s)[:6] == ['kind', 'frames', 'procs', 'median_ms', 'spread_ms', 'a_over_b']


@pytest.mark.parametrize('script', SCRIPTS)
def test_help_needs_neither_torch_nor_the_library(script):
    """`python tools/<script> --help` in a fresh process in which importing torch or cpe_amd raises ImportError"""
    code = ("import runpy, sys; sys.modules['torch'] = sys.modules['cpe_amd'] = None; sys.path.insert(0, sys.argv[1]); "
            "sys.argv = sys.argv[2:]; runpy.run_path(sys.argv[0], run_name='__main__')")
    r = subprocess.run([sys.executable, '-c', code, TOOLS, os.path.join(TOOLS, script + '.py'), '--help'], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert '--child-timeout' in r.stdout and '--procs' in r.stdout
