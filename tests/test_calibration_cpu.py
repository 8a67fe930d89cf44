"""Host logic of the load-time precision calibration (mmf_amd/precision.py), no device: the RoBERTa
precise-mode operand masks the calibration walks (option text_prec_mask: bit k = GEMM kind k -- QKV, out-proj,
FFN-1, FFN-2 -- on hi / lo activations, bit k + 4 = also on W_lo), the option ledger that keeps a set_option /
environment choice out of the calibration's hands, and the helper that runs a batch again after a trap."""
from mmf_amd import precision as P


def test_prec_masks_cover_every_level_cheapest_first():
    ms = P.prec_masks()
    # three levels per kind (fp16 operands, hi / lo activations, + W_lo) for four kinds, minus the full mode
    assert len(ms) == 3 ** 4 - 1 and len(set(ms)) == len(ms)
    assert P.PREC_FULL not in ms and ms[0] == 0
    for m in ms:
        assert 0 <= m < 256
        assert (m >> 4) & ~m & 15 == 0, f"mask {m}: W_lo on a kind without hi / lo activations"
    costs = [P.mask_cost(m) for m in ms]
    assert costs == sorted(costs)
    assert max(costs) < P.mask_cost(P.PREC_FULL)


def test_mask_cost_counts_products_per_kind():
    c = P.PREC_KIND_COST
    assert P.mask_cost(0) == sum(c)                 # one fp16 product per kind
    assert P.mask_cost(P.PREC_FULL) == 3 * sum(c)   # three products per kind
    assert P.mask_cost(1) == sum(c) + c[0]          # QKV on hi / lo activations: two products
    assert P.mask_cost(1 | 16) == sum(c) + 2 * c[0]  # ... and W_lo: three
    assert P.mask_cost(16) == sum(c)                # a W_lo bit without its activation bit is inert


class _Stub:
    def __init__(self, options):
        self.opts = dict(options)

    def get_option(self, name):
        return self.opts[name]

    def set_option(self, name, value):
        self.opts[name] = int(value)


def test_pin_detection():
    s = _Stub({"text_hilo": -1, "effnet_fp32": 0})
    ledger = P.OptionLedger(s)
    assert not ledger.changed("text_hilo")          # never written by the engine: no record, no pin
    ledger.write("text_hilo", -1)
    assert s.opts["text_hilo"] == -1 and not ledger.changed("text_hilo")
    s.set_option("text_hilo", 1)                      # a user's set_option after the engine's write
    assert ledger.changed("text_hilo")
    ledger.write("text_hilo", 2)                      # the engine's own later write clears it
    assert not ledger.changed("text_hilo")
    ledger.record("effnet_fp32")
    assert s.opts["effnet_fp32"] == 0 and ledger.last("effnet_fp32") == 0  # recorded, not written
    assert ledger.last("clip_res16") is None and ledger.last("clip_res16", 1) == 1
    s.set_option("effnet_fp32", 1)
    assert ledger.changed("effnet_fp32")


def test_rerun_if_runs_once_or_twice():
    results = iter(["first", "second"])
    runs, seen = [], []

    def run():
        runs.append(next(results))
        return runs[-1]

    def trap(hit):
        def t(v):
            seen.append(v)
            return hit
        return t
    assert P.rerun_if(trap(False), run) == "first" and runs == ["first"] and seen == ["first"]
    results = iter(["first", "second"])
    del runs[:], seen[:]
    assert P.rerun_if(trap(True), run, probe=str.upper) == "second"
    assert runs == ["first", "second"] and seen == ["FIRST"]  # the trap sees probe(result), once
