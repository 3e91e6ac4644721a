"""A recorder at the one seam between Trainer._adam_step and the library's Adam entry points, engine.adam_update, shared by the CPU
dispatch tests (test_optim_cpu, test_gradclip_cpu, test_accum_cpu).  Nothing is launched.

calls = spy(monkeypatch) -> a list that fills with (name, positional arguments, keyword arguments):
  * an adam_update call as (entry, (p, g, m, v), options): `entry` is the library entry point engine.adam_entry derives from the
    recorded options, without its 'pg_' ('adam_step', 'adamw_step_dev', ...), `options` every keyword of adam_update with its default
    filled in: step, lr, scalars, ema, ema_decay, stat, weight_decay, beta1, beta2, eps;
  * grad_norm / grad_accum as they are called."""


def spy(monkeypatch, others=('grad_norm', 'grad_accum')):
    from patchgan_amd import engine as E
    calls = []

    # (adam_update's own signature: an argument it would refuse is refused here too)
    def adam_update(p, g, m, v, *, step=None, lr=None, scalars=None, ema=None, ema_decay=None, stat=None, weight_decay=None, beta1=0.9,
                    beta2=0.999, eps=1e-8):
        if (step is None) != (lr is None) or (scalars is not None) == (step is not None):
            raise ValueError("adam_update takes either step and lr or scalars")
        entry = E.adam_entry(ema is not None, stat is not None, weight_decay is not None, scalars is not None)
        calls.append((entry[len('pg_'):], (p, g, m, v),
                      dict(step=step, lr=lr, scalars=scalars, ema=ema, ema_decay=ema_decay, stat=stat, weight_decay=weight_decay,
                           beta1=beta1, beta2=beta2, eps=eps)))

    monkeypatch.setattr(E, 'adam_update', adam_update)
    for name in others:
        monkeypatch.setattr(E, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    return calls


def step_lr(call):
    return call[2]['step'], call[2]['lr']


def betas(call):
    return call[2]['beta1'], call[2]['beta2']
