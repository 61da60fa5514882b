"""The loop of realvsr_amd.train with a recording stub model and a list as loader: call order, stop, cadence, resume."""
import pytest

from realvsr_amd import train as T


class Recorder:
    def __init__(self):
        self.calls = []
        self.opt = {}

    def update_learning_rate(self, cur_iter, warmup_iter=-1):
        self.calls.append(('update_learning_rate', cur_iter, warmup_iter))

    def feed_data(self, data):
        self.calls.append(('feed_data', data))

    def optimize_parameters(self, step, log=True):
        self.calls.append(('optimize_parameters', step, log))

    def get_current_log(self):
        return {'l_pix': 0.25}

    def get_current_learning_rate(self):
        return [1e-4, 2e-4]

    def save(self, label):
        self.calls.append(('save', label))

    def save_training_state(self, epoch, step):
        self.calls.append(('save_training_state', epoch, step))

    def resume_training(self, state):
        self.calls.append(('resume_training', state['iter']))


class Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _opt(niter=7, print_freq=2, val_freq=3, save_freq=3, warmup=-1):
    return {'name': 'stub', 'dist': False, 'train': {'niter': niter, 'warmup_iter': warmup, 'val_freq': val_freq},
            'logger': {'print_freq': print_freq, 'save_checkpoint_freq': save_freq}}


@pytest.fixture
def validations(monkeypatch):
    seen = []

    def fake(model, val_set, step, logger=None, tb_logger=None):
        model.calls.append(('validate', step))
        seen.append((val_set, step))
    monkeypatch.setattr(T, 'validate', fake)
    return seen


def test_call_order_cadence_and_stop(validations):
    m, log = Recorder(), Log()
    last = T.train(_opt(), m, ['a', 'b', 'c'], val_set='VAL', logger=log)
    assert last == 7
    want = []
    for step in range(1, 8):
        want += [('update_learning_rate', step, -1), ('feed_data', 'abc'[(step - 1) % 3]), ('optimize_parameters', step, step % 2 == 0)]
        if step % 3 == 0:
            want += [('validate', step), ('save', step), ('save_training_state', (step - 1) // 3, step)]
    want.append(('save', 'latest'))
    assert m.calls == want
    assert validations == [('VAL', 3), ('VAL', 6)]
    lines = [v for v in log.lines if v.startswith('<epoch')]
    assert lines == ['<epoch:{:3d}, iter:{:8,d}, lr:(1.000e-04,2.000e-04,)>, l_pix: 2.5000e-01 '.format((s - 1) // 3, s) for s in (2, 4, 6)]
    assert log.lines[-2:] == ['Saving the final model.', 'End of training.']


def test_no_val_set_no_validation_and_warmup_is_passed_on(validations):
    m = Recorder()
    T.train(_opt(niter=3, warmup=2), m, ['a'] * 5, val_set=None, logger=Log())
    assert validations == [] and [c for c in m.calls if c[0] == 'validate'] == []
    assert [c for c in m.calls if c[0] == 'update_learning_rate'] == [('update_learning_rate', s, 2) for s in (1, 2, 3)]
    assert [c[1] for c in m.calls if c[0] == 'feed_data'] == ['a'] * 3 and m.calls[-1] == ('save', 'latest')


def test_resume_starts_after_the_saved_iteration(validations):
    m, log = Recorder(), Log()
    T.train(_opt(niter=6), m, ['a', 'b', 'c'], val_set='VAL', resume_state={'epoch': 1, 'iter': 3}, logger=log)
    assert m.calls[0] == ('resume_training', 3)
    assert [c[1] for c in m.calls if c[0] == 'optimize_parameters'] == [4, 5, 6]
    assert ('save_training_state', 1, 6) in m.calls and validations == [('VAL', 6)] and m.calls[-1] == ('save', 'latest')
    assert 'Resuming training from epoch: 1, iter: 3.' in log.lines


def test_other_ranks_step_but_do_not_write(validations):
    m, log = Recorder(), Log()
    T.train(_opt(niter=3), m, ['a', 'b', 'c'], val_set='VAL', rank=1, logger=log)
    names = [c[0] for c in m.calls]
    assert names.count('optimize_parameters') == 3 and 'save' not in names and 'validate' not in names
    assert not [v for v in log.lines if v.startswith('<epoch')]


def test_sampler_gets_the_epoch(validations):
    class Sampler:
        epochs = []

        def set_epoch(self, e):
            self.epochs.append(e)
    s = Sampler()
    T.train(_opt(niter=5), Recorder(), ['a', 'b'], train_sampler=s, logger=Log())
    assert s.epochs == [0, 1, 2]
