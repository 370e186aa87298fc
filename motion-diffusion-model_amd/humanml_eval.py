"""The HumanML3D / KIT evaluation loop of the reference's eval/eval_humanml.py -- `evaluate_matching_score`, `evaluate_fid`,
`evaluate_diversity`, `evaluate_multimodality`, `get_metric_statistics`, `evaluation` -- under its signatures, on the metrics of
mdm_amd/humanml_metrics.py.  The same lines are printed in the same order (to stdout and to the log file), and the same dictionaries
come back, with Python floats / numpy arrays as values.

What differs is where the data lives.  Per loader the text and motion embeddings of all batches are concatenated on the device and ONE
`retrieval` call covers every batch (the batch sizes travel as host integers); `activation_dict` holds device tensors, which
`evaluate_fid` and `evaluate_diversity` take as they are.  Nothing is copied to the host per batch; what reaches the host per loader
is four numbers (the matching-score sum and three counts), the D x D statistics for scipy's sqrtm, and one mean per metric.
With the module switch `FID_ON_DEVICE = True` (off by default; a switch and not a keyword, because `evaluate_fid` and `evaluation`
keep the reference's parameter lists) the distance is `hm.frechet_distance_device`'s: the statistics stay on the device and one
scalar comes back.

`eval_wrapper` is any object with the reference's `get_co_embeddings(word_embs=, pos_ohot=, cap_lens=, motions=, m_lens=)` and
`get_motion_embeddings(motions=, m_lens=)` that returns device tensors (mdm_amd.evaluator.EvaluatorMDMWrapper)."""
from collections import OrderedDict
from datetime import datetime

import numpy as np
import torch

from . import humanml_metrics as hm

TOP_K = 3
FID_ON_DEVICE = False      # True: evaluate_fid takes hm.frechet_distance_device(...).item() instead of the host formula (scipy sqrtm)


def _say(line, file):
    print(line)
    print(line, file=file, flush=True)


def evaluate_matching_score(eval_wrapper, motion_loaders, file):
    match_score_dict, R_precision_dict, activation_dict = OrderedDict(), OrderedDict(), OrderedDict()
    print('========== Evaluating Matching Score ==========')
    for motion_loader_name, motion_loader in motion_loaders.items():
        texts, motions_emb, batch_sizes = [], [], []
        with torch.no_grad():
            for batch in motion_loader:
                word_embeddings, pos_one_hots, _, sent_lens, motions, m_lens, _ = batch
                text_embeddings, motion_embeddings = eval_wrapper.get_co_embeddings(word_embs=word_embeddings, pos_ohot=pos_one_hots,
                                                                                    cap_lens=sent_lens, motions=motions, m_lens=m_lens)
                texts.append(text_embeddings)
                motions_emb.append(motion_embeddings)
                batch_sizes.append(int(text_embeddings.shape[0]))
            all_text_embeddings = torch.cat(texts, dim=0)
            all_motion_embeddings = torch.cat(motions_emb, dim=0)
            _, _, topk_count, diag_sum = hm.retrieval(all_text_embeddings, all_motion_embeddings, batch_sizes, TOP_K)
        all_size = sum(batch_sizes)
        matching_score = float(diag_sum.item()) / all_size
        R_precision = topk_count.cpu().numpy() / all_size
        match_score_dict[motion_loader_name] = matching_score
        R_precision_dict[motion_loader_name] = R_precision
        activation_dict[motion_loader_name] = all_motion_embeddings

        _say(f'---> [{motion_loader_name}] Matching Score: {matching_score:.4f}', file)
        _say(f'---> [{motion_loader_name}] R_precision: ' + ''.join('(top %d): %.4f ' % (i + 1, r) for i, r in enumerate(R_precision)), file)
    return match_score_dict, R_precision_dict, activation_dict


def evaluate_fid(eval_wrapper, groundtruth_loader, activation_dict, file):
    eval_dict = OrderedDict()
    gt_motion_embeddings = []
    print('========== Evaluating FID ==========')
    with torch.no_grad():
        for batch in groundtruth_loader:
            _, _, _, sent_lens, motions, m_lens, _ = batch
            gt_motion_embeddings.append(eval_wrapper.get_motion_embeddings(motions=motions, m_lens=m_lens))
    gt_mu, gt_cov = hm.calculate_activation_statistics(torch.cat(gt_motion_embeddings, dim=0))
    for model_name, motion_embeddings in activation_dict.items():
        mu, cov = hm.calculate_activation_statistics(motion_embeddings)
        if FID_ON_DEVICE:
            fid = hm.frechet_distance_device(gt_mu, gt_cov, mu, cov).item()
        else:
            fid = hm.calculate_frechet_distance(gt_mu, gt_cov, mu, cov)
        _say(f'---> [{model_name}] FID: {fid:.4f}', file)
        eval_dict[model_name] = fid
    return eval_dict


def evaluate_diversity(activation_dict, file, diversity_times):
    eval_dict = OrderedDict()
    print('========== Evaluating Diversity ==========')
    for model_name, motion_embeddings in activation_dict.items():
        diversity = float(hm.calculate_diversity(motion_embeddings, diversity_times).item())
        eval_dict[model_name] = diversity
        _say(f'---> [{model_name}] Diversity: {diversity:.4f}', file)
    return eval_dict


def evaluate_multimodality(eval_wrapper, mm_motion_loaders, file, mm_num_times):
    eval_dict = OrderedDict()
    print('========== Evaluating MultiModality ==========')
    for model_name, mm_motion_loader in mm_motion_loaders.items():
        mm_motion_embeddings = []
        with torch.no_grad():
            for batch in mm_motion_loader:
                motions, m_lens = batch                    # (1, mm_replications, ...)
                mm_motion_embeddings.append(eval_wrapper.get_motion_embeddings(motions[0], m_lens[0]).unsqueeze(0))
        if len(mm_motion_embeddings) == 0:
            multimodality = 0
        else:
            multimodality = float(hm.calculate_multimodality(torch.cat(mm_motion_embeddings, dim=0), mm_num_times).item())
        _say(f'---> [{model_name}] Multimodality: {multimodality:.4f}', file)
        eval_dict[model_name] = multimodality
    return eval_dict


def get_metric_statistics(values, replication_times):
    mean = np.mean(values, axis=0)
    std = np.std(values, axis=0)
    conf_interval = 1.96 * std / np.sqrt(replication_times)
    return mean, conf_interval


def evaluation(eval_wrapper, gt_loader, eval_motion_loaders, log_file, replication_times, diversity_times, mm_num_times, run_mm=False,
               eval_platform=None):
    with open(log_file, 'w') as f:
        all_metrics = OrderedDict((name, OrderedDict()) for name in ('Matching Score', 'R_precision', 'FID', 'Diversity', 'MultiModality'))
        for replication in range(replication_times):
            motion_loaders, mm_motion_loaders = {'ground truth': gt_loader}, {}
            for motion_loader_name, motion_loader_getter in eval_motion_loaders.items():
                motion_loaders[motion_loader_name], mm_motion_loaders[motion_loader_name] = motion_loader_getter()

            _say(f'==================== Replication {replication} ====================', f)
            _say(f'Time: {datetime.now()}', f)
            mat_score_dict, R_precision_dict, acti_dict = evaluate_matching_score(eval_wrapper, motion_loaders, f)
            _say(f'Time: {datetime.now()}', f)
            fid_score_dict = evaluate_fid(eval_wrapper, gt_loader, acti_dict, f)
            _say(f'Time: {datetime.now()}', f)
            div_score_dict = evaluate_diversity(acti_dict, f, diversity_times)
            results = [('Matching Score', mat_score_dict), ('R_precision', R_precision_dict), ('FID', fid_score_dict),
                       ('Diversity', div_score_dict)]
            if run_mm:
                _say(f'Time: {datetime.now()}', f)
                results.append(('MultiModality', evaluate_multimodality(eval_wrapper, mm_motion_loaders, f, mm_num_times)))
            _say('!!! DONE !!!', f)
            for metric_name, score_dict in results:
                for key, item in score_dict.items():
                    all_metrics[metric_name].setdefault(key, []).append(item)

        mean_dict = {}
        for metric_name, metric_dict in all_metrics.items():
            _say('========== %s Summary ==========' % metric_name, f)
            for model_name, values in metric_dict.items():
                mean, conf_interval = get_metric_statistics(np.array(values), replication_times)
                mean_dict[metric_name + '_' + model_name] = mean
                if isinstance(mean, (np.float64, np.float32)):
                    _say(f'---> [{model_name}] Mean: {mean:.4f} CInterval: {conf_interval:.4f}', f)
                elif isinstance(mean, np.ndarray):
                    _say(f'---> [{model_name}]' + ''.join('(top %d) Mean: %.4f CInt: %.4f;' % (i + 1, mean[i], conf_interval[i])
                                                         for i in range(len(mean))), f)

        if eval_platform is not None:
            for k, v in mean_dict.items():
                if k.startswith('R_precision'):
                    for i in range(len(v)):
                        eval_platform.report_scalar(name=f'top{i + 1}_' + k, value=v[i], iteration=1, group_name='Eval')
                else:
                    eval_platform.report_scalar(name=k, value=v, iteration=1, group_name='Eval')
        return mean_dict
