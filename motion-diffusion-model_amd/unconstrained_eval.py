"""eval/unconstrained/evaluate.py `evaluate_unconstrained_metrics` on the HIP path: the ST-GCN recogniser (`STGCNUnconstrained`) and
every metric behind it (`mdm_amd.metrics`) run on the device, so the features never leave it and precision / recall is no longer the
part a `fast` run has to skip.  Same root-joint centring, batches of 64, order of the random draws (KID, then the diversity of the
dataset, then of the generated motions) and result dictionary as upstream.  Differences: the caller's `generated_motions` is not
modified (upstream centres it in place); the batches are slices, not a DataLoader with worker processes; the progress prints are gone;
`fid_on_device=True` (off by default) takes the FID from `metrics.calculate_fid_device` instead of scipy's sqrtm on the host."""
import numpy as np
import torch

from . import metrics
from .stgcn import STGCNUnconstrained

ACT_REC_MODEL_PATH = "./assets/actionrecognition/humanact12_gru_modi_struct.pth.tar"
DATASET_PATH = "./dataset/HumanAct12Poses/humanact12_unconstrained_modi_struct.npy"
BATCH_SIZE = 64
ROOT_JOINT = 8
NUM_CLASSES = 12


def initialize_model(device, modelpath):
    model = STGCNUnconstrained(in_channels=3, num_class=NUM_CLASSES, graph_args={"layout": "openpose", "strategy": "spatial"},
                               edge_importance_weighting=True, device=device)
    model = model.to(device)
    model.load_state_dict(torch.load(modelpath, map_location=device))
    model.eval()
    return model


def centre_root(motions):
    """[N, V, 3, T] with the root joint of every frame at the origin, as a new fp32 tensor (on the motions' device)."""
    m = (motions if torch.is_tensor(motions) else torch.from_numpy(np.asarray(motions))).float()
    if m.dim() != 4:
        raise ValueError(f"motions must be [N, joints, 3, frames], got {tuple(m.shape)}")
    return m - m[:, ROOT_JOINT:ROOT_JOINT + 1, :, :]


def compute_features(model, motions, device):
    """(features [N, 256], yhat [N, num_class]) on `device`, in batches of 64."""
    activations, predictions = [], []
    with torch.no_grad():
        for n0 in range(0, len(motions), BATCH_SIZE):
            batch = {"x": motions[n0:n0 + BATCH_SIZE].to(device).float()}
            model(batch)
            activations.append(batch["features"].reshape(batch["yhat"].shape[0], -1))      # (forward squeezes a batch of one)
            predictions.append(batch["yhat"])
    return torch.cat(activations, dim=0), torch.cat(predictions, dim=0)


def evaluate_unconstrained_metrics(generated_motions, device, fast, act_rec_model_path=ACT_REC_MODEL_PATH, dataset_path=DATASET_PATH,
                                   kid_subsets=metrics.KID_SUBSETS, kid_subset_size=metrics.KID_SUBSET_SIZE, fid_on_device=False):
    act_rec_model = initialize_model(device, act_rec_model_path)

    generated_features, _ = compute_features(act_rec_model, centre_root(generated_motions), device)
    generated_stats = metrics.calculate_activation_statistics(generated_features)

    motion_data = np.load(dataset_path, allow_pickle=True)[:, :15]      # (the file keeps a 16th joint of an older format)
    dataset_features, _ = compute_features(act_rec_model, centre_root(motion_data), device)
    real_stats = metrics.calculate_activation_statistics(dataset_features)

    if fid_on_device:
        fid = metrics.calculate_fid_device(generated_stats, real_stats).item()
    else:
        fid = metrics.calculate_fid(generated_stats, real_stats)
    kid = metrics.calculate_kid(dataset_features, generated_features, n_subsets=kid_subsets, subset_size=kid_subset_size)
    dataset_diversity = metrics.calculate_diversity(dataset_features)
    generated_diversity = metrics.calculate_diversity(generated_features)
    if fast:
        precision = recall = None
    else:
        precision, recall = metrics.precision_and_recall(generated_features, dataset_features)
    return {"fid": fid, "kid": kid[0], "diversity_gen": generated_diversity.cpu().item(), "diversity_gt": dataset_diversity.cpu().item(),
            "precision": precision, "recall": recall}
