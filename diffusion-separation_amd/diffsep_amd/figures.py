"""figures.py — the reference's figure of the reverse diffusion (evaluate.py:29-61, `fig/<split>/evo_NNN.pdf`; the paper's
figure_reverse_diffusion_example.py draws the same picture): the state of n_fig reverse steps next to the clean sources, one
row per source, as spectrograms.  The states come from the fused sampler's tap (Engine.pc_sample(snapshots=...)); the
spectrogram and the PDF are matplotlib's, on the host — rendering the PDF is by far most of the cost.  matplotlib is
imported here and nowhere else, with the Agg backend and through its object interface (no pyplot state: no window, and
nothing that another thread's figure could touch).
"""
import numpy as np

N_FIG = 6  # panels of the reference's figure (evaluate.py:29)


def panel_steps(N, n_fig=N_FIG):
    """The reverse steps the reference draws out of N (evaluate.py:37): round(linspace(0, 1, n_fig) (N - 1)), numpy's
    half-to-even rounding — 0, 6, 12, 17, 23, 29 for N = 30.  For N < n_fig steps repeat."""
    return np.round(np.linspace(0, 1, n_fig) * (N - 1)).astype(np.int64)


def snapshot_request(N, n_fig=N_FIG):
    """-> (steps, panel_of): the unique panel steps, strictly ascending (what the sampler's tap is asked for), and for every
    panel the index of its step in that list."""
    panels = [int(s) for s in panel_steps(N, n_fig)]
    steps = sorted(set(panels))
    return steps, [steps.index(s) for s in panels]


def panel_time(N, step):
    """the title's diffusion time of a panel: (N - 1 - step) / (N - 1), from 1 at the first step down to 0 (N = 1: 1)"""
    return 1.0 if N <= 1 else (N - 1 - step) / (N - 1)


def require_matplotlib(flag="--fig"):
    """SystemExit naming matplotlib when it cannot be imported (called before any GPU work)"""
    try:
        import matplotlib  # noqa: F401
    except ImportError as err:
        raise SystemExit(f"{flag} draws with matplotlib, which cannot be imported here ({err})")


def evolution_figure(states, steps, N, target, path, vmin=-75, vmax=0, noise_seed=0):
    """states [n_fig, S, T]: the state of the panels' reverse steps, sources in the targets' order; steps [n_fig]: their step
    numbers out of N; target [S, T]: the clean sources.  Writes the reference's figure to `path` (evaluate.py:29-61:
    Axes.specgram defaults, vmin / vmax, titles t = (N - 1 - step) / (N - 1), a last column "clean" with 1e-10 noise added —
    here from a Generator of its own, seeded with noise_seed, so that a figure does not depend on what else drew numbers —
    and one colour bar).  Returns {"axes": number of axes, "clean": the S rows drawn in the last column}."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    states, target = np.asarray(states, dtype=np.float64), np.asarray(target, dtype=np.float64)
    n_fig, S, _ = states.shape
    assert len(steps) == n_fig and target.shape[0] == S
    fig = Figure(figsize=(20, 2 * S))
    FigureCanvasAgg(fig)
    axes = fig.subplots(S, n_fig + 1, squeeze=False)
    rng = np.random.default_rng(noise_seed)
    im, clean = None, []
    with np.errstate(divide="ignore"):  # (an all-zero row: specgram takes log10 of 0, the panel is empty)
        for idx, step in enumerate(steps):
            for i in range(S):
                axes[i, idx].specgram(states[idx, i], vmin=vmin, vmax=vmax)
                axes[i, idx].set_xticks([])
                axes[i, idx].set_yticks([])
                if i == 0:
                    axes[i, idx].set_title(f"t={panel_time(N, int(step)):.2f}")
        for i in range(S):
            tgt = target[i] + rng.standard_normal(target[i].shape) * 1e-10
            clean.append(tgt)
            *_, im = axes[i, -1].specgram(tgt, vmin=vmin, vmax=vmax)
            axes[i, -1].set_xticks([])
            axes[i, -1].set_yticks([])
            if i == 0:
                axes[i, -1].set_title("clean")
        fig.tight_layout()
        fig.subplots_adjust(right=0.8)
        cbar_ax = fig.add_axes([0.85, 0.15, 0.05, 0.7])
        fig.colorbar(im, cax=cbar_ax)
        fig.savefig(path, format="pdf")
    return {"axes": len(fig.axes), "clean": clean}
