"""CPU tests of the wiring of the built-in SSIM term: model.loss.perceptual_name decides what DifferentiableBlocksWorld._init_loss installs
as perceptual_fn ('ssim' with a positive weight: metrics.SSIMTerm; 'lpips', a missing key or a zero weight: nothing, set_perceptual is
needed as before), set_perceptual overrides it, the key survives init_kwargs (a model rebuilt from a checkpoint has the term again), and
python -m dbw_amd.train settles the term from the config's key, --perceptual, the LPIPS weight files and --no-perceptual.  The prototypes of
the two new entry points are held against the binding and the library's exports by tests/test_abi_families.py."""
import os

import pytest
import torch

import dbw_amd
from dbw_amd import metrics, train

CONFIGS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'configs', 'dtu')


def _cfg(**loss):
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': 2, 'txt_size': 8},
                      'renderer': {'faces_per_pixel': 2, 'cameras': {'name': 'perspective'}},
                      'rend_optim': {'decouple_rendering': True}, 'loss': dict(rgb_weight=1, **loss)}}


def _model(**loss):
    torch.manual_seed(0)
    return dbw_amd.create_model(_cfg(**loss), (16, 24))


def test_perceptual_name_ssim_installs_the_term():
    m = _model(perceptual_name='ssim', perceptual_weight=0.1)
    assert m.perceptual_name == 'ssim' and isinstance(m.perceptual_fn, metrics.SSIMTerm)
    assert m.loss_weights['perceptual'] == 0.1 and 'loss_perceptual' in m.loss_names
    assert not any(k.startswith('perceptual_fn') for k in m.state_dict())          # no parameters, nothing in a checkpoint
    a, b = torch.rand(2, 3, 16, 24), torch.rand(2, 3, 16, 24)
    want = (1 - metrics.ssim_map(a, b, padding=True)).mean()
    assert torch.equal(m.perceptual_fn(a, b), want)                                 # (CPU tensors: the torch formula)


def test_other_names_install_nothing():
    for loss in (dict(perceptual_name='lpips', perceptual_weight=0.1), dict(perceptual_weight=0.1), dict(perceptual_name='ssim'),
                 dict(perceptual_name='ssim', perceptual_weight=0)):
        m = _model(**loss)
        assert m.perceptual_fn is None and m.perceptual_name == loss.get('perceptual_name', 'lpips')
    m = _model(perceptual_weight=0.1)
    with pytest.raises(RuntimeError, match='set_perceptual'):
        m._perceptual_term(torch.rand(1, 3, 16, 24), torch.rand(1, 3, 16, 24), coarse=False)


def test_set_perceptual_overrides():
    m = _model(perceptual_name='ssim', perceptual_weight=0.1)
    fn = lambda imgs, rec: (imgs - rec).abs().mean()
    m.set_perceptual(fn)
    assert m.perceptual_fn is fn
    net = torch.nn.Conv2d(3, 1, 1)
    m.set_perceptual(net)
    assert m.perceptual_fn is net
    m.set_perceptual(None)
    assert m.perceptual_fn is None


def test_init_kwargs_round_trip():
    m = _model(perceptual_name='ssim', perceptual_weight=0.1)
    kw = m.init_kwargs
    assert kw['loss']['perceptual_name'] == 'ssim' and kw['loss']['perceptual_weight'] == 0.1
    again = dbw_amd.DifferentiableBlocksWorld(**kw)
    assert isinstance(again.perceptual_fn, metrics.SSIMTerm) and again.init_kwargs == kw
    again.load_state_dict(m.state_dict())


def test_the_command_line_settles_the_term(tmp_path, capsys):
    base = ['--config', os.path.join(CONFIGS, 'scan24.yml'), '--tag', 't', '--data-root', str(tmp_path), '--runs-root', str(tmp_path / 'runs')]
    cfg = train.prepare_config(train.parse_args(base + ['--perceptual', 'ssim']))          # a shipped config as it is, no weight files
    assert cfg['model']['loss']['perceptual_name'] == 'ssim' and cfg['model']['loss']['perceptual_weight'] == 0.1
    for files in (['--lpips-vgg', 'X'], ['--lpips-lin', 'Y'], ['--lpips-vgg', 'X', '--lpips-lin', 'Y']):
        with pytest.raises(SystemExit) as e:
            train.prepare_config(train.parse_args(base + ['--perceptual', 'ssim'] + files))
        assert 'ssim' in str(e.value) and '--lpips-vgg' in str(e.value) and 'contradict' in str(e.value)
    with pytest.raises(SystemExit) as e:                                                     # the plain config: the old words, and the new flag
        train.prepare_config(train.parse_args(base))
    assert 'perceptual_weight = 0.1' in str(e.value) and '--lpips-vgg' in str(e.value) and '--no-perceptual' in str(e.value)
    assert '--perceptual ssim' in str(e.value)
    with pytest.raises(SystemExit):                                                          # --perceptual lpips overrides a config's ssim
        train.prepare_config(train.parse_args(base + ['--perceptual', 'lpips']))
    (tmp_path / 'default.yml').write_text(open(os.path.join(CONFIGS, 'default.yml')).read())
    (tmp_path / 'own.yml').write_text('dataset:\n  name: dtu\n  tag: scan24\nmodel:\n  loss:\n    perceptual_name: ssim\n')
    own = ['--config', str(tmp_path / 'own.yml')] + base[2:]
    cfg = train.prepare_config(train.parse_args(own))                                        # the key in the config: no flag needed
    assert cfg['model']['loss']['perceptual_name'] == 'ssim' and cfg['model']['loss']['perceptual_weight'] == 0.1
    with pytest.raises(SystemExit):
        train.prepare_config(train.parse_args(own + ['--lpips-vgg', 'X', '--lpips-lin', 'Y']))
    with pytest.raises(SystemExit) as e:
        train.prepare_config(train.parse_args(own + ['--perceptual', 'lpips']))
    assert 'perceptual_weight = 0.1' in str(e.value)
    capsys.readouterr()
    cfg = train.prepare_config(train.parse_args(base + ['--perceptual', 'ssim', '--no-perceptual']))     # --no-perceptual wins
    assert cfg['model']['loss']['perceptual_weight'] == 0 and 'perceptual_weight 0.1 -> 0' in capsys.readouterr().out
    with pytest.raises(SystemExit):                                                          # (argparse: not one of the two names)
        train.parse_args(base + ['--perceptual', 'vgg'])
    assert not (tmp_path / 'runs').exists()
