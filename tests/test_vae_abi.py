"""The VAE entry points of the C ABI (csrc/vae.hip), checked without a GPU: exported, bound, and every argument-validation case
returns UNETRIR_EINVAL (10001) before the device is touched."""
NEW = ("unetrir_normal_f32", "unetrir_normal_dev_f32", "unetrir_vae_sample_kl_fwd_f32", "unetrir_vae_sample_kl_bwd_f32",
       "unetrir_vae_loss_add_f32")
EINVAL = 10001
P = 0x7F0000001000          # a non-null, 16-byte aligned address: validation must return before anything dereferences it


def _lib():
    import unet_rir_amd
    return unet_rir_amd, unet_rir_amd._lib.lib()


def test_new_symbols_are_exported_bound_and_wrapped():
    U, L = _lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in U._lib.EXPORTS, n
    for n in ("normal", "normal_dev", "vae_sample_kl_fwd", "vae_sample_kl_bwd", "vae_loss_add"):
        assert callable(getattr(U.ops, n)), n
    assert L.unetrir_abi_version() == 1
    assert U.VAE.ENGINE is U.VAEEngine


def test_normal_argument_validation():
    _, L = _lib()
    assert L.unetrir_normal_f32(None, 16, 1, 0, None) == EINVAL
    assert L.unetrir_normal_f32(P, 0, 1, 0, None) == EINVAL
    assert L.unetrir_normal_f32(P, -4, 1, 0, None) == EINVAL
    assert L.unetrir_normal_dev_f32(None, 16, 1, P, 0, None) == EINVAL
    assert L.unetrir_normal_dev_f32(P, 16, 1, None, 0, None) == EINVAL          # no device counter to read
    assert L.unetrir_normal_dev_f32(P, 0, 1, P, 0, None) == EINVAL


def _fwd(L, mu=P, ld_mu=8, lv=P, ld_lv=8, eps=P, B=2, L_=8, z=P, ld_z=8, kl=P):
    return L.unetrir_vae_sample_kl_fwd_f32(mu, ld_mu, lv, ld_lv, eps, B, L_, 0.5, z, ld_z, kl, None)


def test_sample_kl_fwd_argument_validation():
    _, L = _lib()
    for kw in (dict(mu=None), dict(lv=None), dict(eps=None), dict(z=None), dict(kl=None),          # null pointers
               dict(B=0), dict(B=-1), dict(L_=0), dict(L_=-8),                                      # B or L <= 0
               dict(L_=6), dict(L_=7),                                                              # L not a multiple of 4
               dict(ld_mu=4), dict(ld_lv=4), dict(ld_z=4)):                                         # a row stride shorter than L
        assert _fwd(L, **kw) == EINVAL, kw


def _bwd(L, mu=P, ld_mu=8, lv=P, ld_lv=8, eps=P, dz=P, ld_dz=8, B=2, L_=8, dmu=P, ld_dmu=8, dlv=P, ld_dlv=8):
    return L.unetrir_vae_sample_kl_bwd_f32(mu, ld_mu, lv, ld_lv, eps, dz, ld_dz, B, L_, 0.5, dmu, ld_dmu, dlv, ld_dlv, None)


def test_sample_kl_bwd_argument_validation():
    _, L = _lib()
    for kw in (dict(mu=None), dict(lv=None), dict(eps=None), dict(dz=None), dict(dmu=None), dict(dlv=None),
               dict(B=0), dict(B=-3), dict(L_=0), dict(L_=-4), dict(L_=10),
               dict(ld_mu=4), dict(ld_lv=4), dict(ld_dz=4), dict(ld_dmu=4), dict(ld_dlv=4)):
        assert _bwd(L, **kw) == EINVAL, kw


def test_loss_add_argument_validation():
    _, L = _lib()
    assert L.unetrir_vae_loss_add_f32(None, P, None) == EINVAL
    assert L.unetrir_vae_loss_add_f32(P, None, None) == EINVAL
