"""Host logic of the grouped one-shot backward: which convs ``bwd_plans`` routes to it and
which (dgrad, wgrad) plans the pair table holds (no GPU: the pair table is host code)."""
ARGS = (3, 3, (1, 1), (1, 1))


def test_plan_selection(monkeypatch):
    from kubeml_amd.ops import kernels as K
    # layer3: unrolled 2x2-map conv, 1x1 form K = 1024 -> one-shot dgrad + folded wgrad, grouped
    for B in (256, 40, 1):
        d, w, grouped = K.bwd_plans((B, 2, 2, 256), 256, *ARGS, unroll=True)
        assert (d[4], w[4], grouped) == (K.ONESHOT, K.FOLD22, True)
        assert (d[2] & ~1) == 1024 and w[:3] == (16, 16, 256)
    # layer4: centre tap on a 1x1 map, K = 512 -> one-shot dgrad + one-shot wgrad, grouped
    d, w, grouped = K.bwd_plans((256, 1, 1, 512), 512, *ARGS)
    assert (d, w, grouped) == ((32, 32, 512, 1, K.ONESHOT), (32, 32, 256, 1, K.ONESHOT), True)
    # not eligible: more pixels than the panel depth, the 1x1-form scratch, other widths, other maps
    assert K.bwd_plans((512, 2, 2, 256), 256, *ARGS, unroll=True)[1][4] != K.FOLD22
    assert K.bwd_plans((257, 1, 1, 512), 512, *ARGS)[0][4] != K.ONESHOT
    assert K.bwd_plans((256, 2, 2, 256), 256, *ARGS, unroll=True, scratch=True)[1][4] == 0
    assert K.bwd_plans((256, 2, 2, 128), 128, *ARGS, unroll=True)[1][4] != K.FOLD22
    assert K.bwd_plans((256, 4, 4, 128), 128, *ARGS)[0][4] != K.ONESHOT
    assert K.bwd_plans((256, 1, 1, 512), 512, *ARGS, oneshot_pair=False)[0][4] != K.ONESHOT
    # forced plans are taken as given
    assert K.bwd_plans((256, 1, 1, 512), 512, *ARGS, dcfg=(32, 32, 64, 1, 0), wcfg=(32, 32, 64, 1, 0))[0] == \
        (32, 32, 64, 1, 0)
    # the switch, and the two-launch one-shot route keeping its meaning
    monkeypatch.setattr(K, "_ONESHOT_PAIR_ON", False)
    assert K.bwd_plans((256, 2, 2, 256), 256, *ARGS, unroll=True)[1][4] == 0
    assert K.bwd_plans((256, 1, 1, 512), 512, *ARGS)[0][4] != K.ONESHOT
    monkeypatch.setattr(K, "_ONESHOT_PAIR_ON", True)
    monkeypatch.setattr(K, "_ONESHOT_BWD_ON", True)
    d, w, _ = K.bwd_plans((256, 2, 2, 256), 256, *ARGS, unroll=True)
    assert d == (32, 32, 0, 1, K.ONESHOT) and w == (32, 32, 0, 1, K.ONESHOT)


def test_pair_table_matches_variants():
    from kubeml_amd.ops import kernels as K
    for plans in (K._ONESHOT_PAIR_U22_FULL, K._ONESHOT_PAIR_U22_HALF):
        assert K.conv_pair_supported(*plans)
    assert K.conv_pair_supported((32, 32, 512, 1, K.ONESHOT), (32, 32, 256, 1, K.ONESHOT))
    assert K.conv_pair_supported((32, 32, 64, 1, 0), (32, 32, 64, 1, 0))
    # a wgrad variant is part of the key now: the register-staged list entries need variant 0
    assert not K.conv_pair_supported((32, 32, 64, 1, 0), (32, 32, 64, 1, K.ONESHOT))
    assert not K.conv_pair_supported((32, 32, 512, 1, K.ONESHOT), (16, 16, 256, 1, K.FOLD22))
    assert not K.conv_pair_supported((32, 32, 1024, 1, K.ONESHOT), (32, 32, 64, 1, 0))
