"""The launches of one Autoencoder / VAE train step at main_training.py's own size (main_training.py:118-129, :142-152; the geometry
profiles/vae_step.json times): 144 x 160 input, batch 32, filters (64, 128, 256, 512), kernels 3, strides 2, latent 64, n_neurons 2048.

ONE table serves two tests: tests/test_fullsize_ae_vae_gpu.py runs every entry against the fp64 oracle over its whole output, and
tests/test_ae_vae_cases.py builds AutoencoderEngine and VAEEngine on the simulated runtime and asserts that `launches()` below is
exactly the set of (operator, geometry) pairs one forward + backward pass issues - a layer added to either engine is then uncovered
until it is added here (and so to the GPU test)."""
B, H, W = 32, 144, 160
FILTERS, LATENT, N_NEURONS, N_IDX, EMB_DIM = (64, 128, 256, 512), 64, 2048, 32, 256
N_FEAT = 9 * 10 * 512                    # Flatten of the bottleneck
N_CAT = N_FEAT + N_NEURONS               # concatenate([Flatten(x), y]): 48 128

# Conv2D 3x3 stride 2: (real Cin, Cout, H, W); Cin = 2 is stored zero-padded to PAD channels, and its data gradient is never launched
CONV_LAYERS = [(2, 64, 144, 160), (64, 128, 72, 80), (128, 256, 36, 40), (256, 512, 18, 20)]
# Conv2DTranspose 3x3: (stride, Cin, real Cout, h, w) of the INPUT grid; Cout = 2 is stored zero-padded to PAD channels (the output layer)
CONVT_LAYERS = [(1, 512, 512, 9, 10), (2, 512, 256, 9, 10), (2, 256, 128, 18, 20), (2, 128, 64, 36, 40), (2, 64, 2, 72, 80)]
# Dense (fp32 in both storage modes): (K, N) of encoder_inf_dense, encoder_output / mu / log_variance, decoder_dense
DENSE_LAYERS = [(N_IDX * EMB_DIM, N_NEURONS), (N_CAT, LATENT), (LATENT, N_FEAT)]
# BatchNormalization -> ReLU (encoder; Autoencoder decoder) / LeakyReLU (VAE decoder): (C, P)
BN_PAIRS = [(64, B * 72 * 80), (128, B * 36 * 40), (256, B * 18 * 20), (512, B * 9 * 10)]
RELU, LEAKY = 1, 2


def pad(dtype):
    """Stored channels of the 2-channel network input and output: one 16-byte granule."""
    return 8 if dtype == "bf16" else 4


def conv_geom(layer, dtype):
    """(B, H, W, stored Cin, Cout, k, stride) of a CONV_LAYERS entry."""
    ci, co, h, w = layer
    return (B, h, w, pad(dtype) if ci == 2 else ci, co, 3, 2)


def convt_geom(layer, dtype):
    """(B, h, w, Cin, stored Cout, k, stride) of a CONVT_LAYERS entry."""
    s, ci, co, h, w = layer
    return (B, h, w, ci, pad(dtype) if co == 2 else co, 3, s)


def dense_geom(K, N):
    return (B, 1, 1, K, N, 1, 1)


def launches(model, dtype):
    """The set of (operator, geometry...) pairs of one forward + backward pass of `model` ("ae" | "vae") in storage mode `dtype`
    ("f32" | "bf16").  Convolutions carry the storage type of their input; the Dense branch is fp32 in both modes."""
    out = set()
    for layer in CONV_LAYERS:
        g = conv_geom(layer, dtype)
        out |= {("conv2d_fwd", dtype) + g, ("conv2d_wgrad", dtype) + g}
        if layer[0] != 2:                                  # the network input needs no gradient
            out.add(("conv2d_dgrad", dtype) + g)
        if dtype == "f32":
            out.add(("transpose_weight", g[4], 9, g[3]))
    for layer in CONVT_LAYERS:
        g = convt_geom(layer, dtype)
        out |= {("conv2d_transpose_fwd", dtype) + g, ("conv2d_transpose_dgrad", dtype) + g, ("conv2d_transpose_wgrad", dtype) + g}
        if dtype == "f32":
            out.add(("transpose_weight", g[3], 9, g[4]))
    out.add(("colsum", dtype, B * H * W, pad(dtype)))       # bias gradient of the output layer (the only one not in front of BatchNorm)
    for K, N in DENSE_LAYERS:
        out |= {("dense_fwd", B, K, N, True), ("dense_fwd", B, N, K, False), ("conv2d_wgrad", "f32") + dense_geom(K, N),
                ("transpose_weight", N, 1, K), ("colsum", "f32", B, N)}
    if model == "vae":       # mu and log_variance both read the concatenation: the second data gradient adds into the first
        out.add(("conv2d_dgrad_addend", "f32") + dense_geom(N_CAT, LATENT))
    for i, (C, P) in enumerate(BN_PAIRS):
        acts = {RELU, LEAKY} if model == "vae" else {RELU}
        for act in acts:
            out |= {("bn_act", dtype, C, P, act), ("bn_bwd", dtype, C, P, act)}
    return out
