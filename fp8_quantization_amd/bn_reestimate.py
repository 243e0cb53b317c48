"""BN statistics re-estimation of a quantized model (reference: utils/qat_utils.py:60-108, run by
`validate-quantized` before it evaluates unless --no-reestimate-bn-stats, image_net.py:165-168).

The protocol: model.eval(); every BN-fused layer -- the layer itself, not its children -- is put in
training mode with momentum 1, so that after each forward its running buffers hold that batch's
statistics; those are summed per layer over `num_batches` batches; the running buffers become
sum / batch count; momentum is restored and the model is back in eval mode.

On a HIP model the training-mode forward of BNFusedHijacker runs on the deterministic kernels of
csrc/bn_train.h (quantized_folded_bn.py: fuse_bn_train), so two runs -- and every rank of a sharded
run -- end with identical bytes; the statistics feed every later layer's quantizer through
discontinuous rounding, and MIOpen's training batch norm is not reproducible in its last bits.

Layers are recognised by class (`classes`) or by duck type (running_mean, running_var, gamma,
momentum, run_forward), which also matches the reference's own BNFusedHijacker when a model is
built from its operators (INTEGRATION.md route A).
"""
import torch

_DUCK = ("running_mean", "running_var", "gamma", "momentum", "run_forward")


def bn_fused_layers(model, classes=None):
    """[(name, module)] of the model's BN-fused layers: instances of `classes` when given (a class or
    a tuple), else BNFusedHijacker instances and anything with its duck type."""
    from .quantization.quantized_folded_bn import BNFusedHijacker
    out = []
    for name, m in model.named_modules():
        if classes is not None:
            hit = isinstance(m, classes)
        else:
            hit = isinstance(m, BNFusedHijacker) or all(hasattr(m, a) for a in _DUCK)
        if hit:
            out.append((name, m))
    return out


def reestimate_bn_stats(model, batches, num_batches=50, store_ema_stats=False, group=None, classes=None):
    """reestimate_BN_stats (qat_utils.py:60-108).  `batches`: an iterable of inputs, or of (input, ...)
    tuples as a data loader yields; inputs are moved to the model's device.  Returns the number of
    batches that entered the average (over all ranks).

    num_batches < 1 raises ValueError: the reference stops on `batch_count == num_batches`, which 0
    never meets, so it would walk the whole loader -- an accident of that test, not a protocol.

    store_ema_stats keeps the previous statistics in the buffers running_mean_ema / running_var_ema
    (registered on first use, refreshed afterwards), as the reference does.

    Multi-GPU -- `group` given, or torch.distributed initialised (then the default group): rank r
    runs the batches r, r + world, ... of the first `num_batches`; the per-layer sums of all layers
    and the batch count travel in one flat float32 buffer, all-reduced once
    (distributed.allreduce_bn_sums); every rank divides, and all ranks end with identical bytes.

    The running buffers are updated in place (the reference rebinds them): the fused eval store's
    cached scale / shift (BNFusedHijacker._bn_act_cache) is keyed on the buffers' version counters,
    so the eval forward that follows picks the new statistics up."""
    import torch.distributed as dist
    from .distributed import allreduce_bn_sums
    num_batches = int(num_batches)
    if num_batches < 1:
        raise ValueError(f"reestimate_bn_stats: num_batches must be at least 1, got {num_batches}")
    world, rank = 1, 0
    if dist.is_available() and dist.is_initialized():
        world, rank = dist.get_world_size(group), dist.get_rank(group)
    layers = bn_fused_layers(model, classes)
    model.eval()
    org_momentum = {}
    with torch.no_grad():
        for name, m in layers:
            org_momentum[name] = m.momentum
            m.momentum = 1.0
            m.running_mean_sum = torch.zeros_like(m.running_mean)
            m.running_var_sum = torch.zeros_like(m.running_var)
            m.training = True  # the layer alone, not its children
            if store_ema_stats:
                if not hasattr(m, "running_mean_ema"):
                    m.register_buffer("running_mean_ema", m.running_mean.detach().clone())
                    m.register_buffer("running_var_ema", m.running_var.detach().clone())
                else:
                    m.running_mean_ema = m.running_mean.detach().clone()
                    m.running_var_ema = m.running_var.detach().clone()
        batch_count = 0
        if layers:
            p0 = next(iter(model.parameters()), None)
            device = p0.device if p0 is not None else None
            for i, b in enumerate(batches):
                if i >= num_batches:
                    break
                if i % world != rank:
                    continue
                x = b[0] if isinstance(b, (tuple, list)) else b
                model(x.to(device) if device is not None else x)
                for _, m in layers:
                    m.running_mean_sum += m.running_mean
                    m.running_var_sum += m.running_var
                batch_count += 1
            sums = [t for _, m in layers for t in (m.running_mean_sum, m.running_var_sum)]
            if world > 1:
                batch_count = allreduce_bn_sums(sums, batch_count, group)
        for name, m in layers:
            if batch_count:
                m.running_mean.copy_(m.running_mean_sum / batch_count)
                m.running_var.copy_(m.running_var_sum / batch_count)
            m.momentum = org_momentum[name]  # (running_*_sum stay on the layer, as in the reference)
    model.eval()
    return batch_count
