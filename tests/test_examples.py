"""The examples/ demos run end to end on 2 CPU ranks through the launcher."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("script,args,expect", [
    ("examples/cluster/demo_kclustering.py", [], "clusters recovered exactly: True"),
    ("examples/classification/demo_knn.py", [], "fold accuracies"),
    ("examples/lasso/demo.py", [], "lambda="),
    ("examples/nn/mnist.py", ["--epochs", "1", "--samples", "512"], "epoch 0"),
    ("examples/nn/imagenet.py", ["--epochs", "2", "--samples", "256", "--batch-size", "16", "--image-size", "32",
                                 "--width", "8", "--classes", "10", "--layers", "1,1"], '"example": "imagenet"'),
    ("examples/nn/imagenet-DASO.py", ["--epochs", "3", "--samples", "256", "--batch-size", "16", "--image-size",
                                      "32", "--width", "8", "--classes", "10", "--layers", "1,1"],
     '"example": "imagenet-DASO"'),
])
def test_example(script, args, expect):
    env = dict(os.environ, HEAT_COMM_BACKEND="gloo", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-m", "heat_amd.run", "-n", "2", "--backend", "gloo",
                          os.path.join(REPO, script)] + args, cwd=REPO, env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert expect in res.stdout


def test_datasets():
    import numpy as np
    import heat_amd as ht

    X, y = ht.datasets.iris()
    assert X.shape == (150, 4) and y.shape == (150,)
    assert np.bincount(y.numpy()).tolist() == [50, 50, 50]
    km = ht.cluster.KMeans(n_clusters=3, init="kmeans++", random_state=1).fit(X)
    assert km.cluster_centers_.shape == (3, 4)
    Xd, yd = ht.datasets.diabetes(synthetic=True)
    assert Xd.shape == (442, 11) and yd.shape == (442, 1)   # same layout as the fixture
    assert np.all(Xd.numpy()[:, 0] == 1.0)
    Xs, ys = ht.datasets.iris(synthetic=True)
    assert Xs.shape == (150, 4) and np.bincount(ys.numpy()).tolist() == [50, 50, 50]


def test_dataset_fixtures(monkeypatch):
    """The reference fixtures (the copies under tests/golden/datasets, found through
    $HEAT_DATASETS_DIR) load through every format with the same values, on every split axis;
    iris() / diabetes() return them."""
    import numpy as np
    import pytest
    import heat_amd as ht

    monkeypatch.setenv("HEAT_DATASETS_DIR", os.path.join(REPO, "tests", "golden", "datasets"))
    ref = np.loadtxt(ht.datasets.fixture_path("iris.csv"), delimiter=";", dtype=np.float32)
    assert ref.shape == (150, 4)
    for name in ("iris.csv", "iris.h5", "iris.nc"):
        for split in (None, 0, 1):
            a = ht.datasets.load_fixture(name, split=split)
            assert a.split == split and a.shape == (150, 4)
            np.testing.assert_allclose(a.numpy(), ref, rtol=1e-6)
    X, y = ht.datasets.iris(split=0)
    np.testing.assert_allclose(X.numpy(), ref, rtol=1e-6)
    # Fisher's iris: class means of petal length are ~1.46 / 4.26 / 5.55 (rows ordered by class)
    pl = ref[:, 2].reshape(3, 50).mean(1)
    np.testing.assert_allclose(pl, [1.46, 4.26, 5.55], atol=5e-3)
    Xd, yd = ht.datasets.diabetes(split=0)
    assert Xd.shape == (442, 11) and yd.shape == (442, 1)
    assert np.allclose(Xd.numpy()[:, 0], 1.0) or Xd.numpy().std(0).min() >= 0
    train = ht.datasets.load_fixture("iris_X_train.csv", split=0)
    assert train.shape == (75, 4)
    with pytest.raises(FileNotFoundError):
        ht.datasets.load_fixture("no_such_fixture.csv")
