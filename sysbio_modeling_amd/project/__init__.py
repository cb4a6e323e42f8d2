from .base_project import Project
from . import utils
from .ensembles import (EnsembleTrajectories, autocorrelation, ensemble_diagnostics, ensemble_predictions, ensemble_trajs,
                        net_ensemble_trajs, pca_eig, pca_eig_log_params, temperature_ladder, traj_ensemble_quantiles,
                        traj_ensemble_stats)
from .profiles import profile_confidence_intervals, profile_likelihood_batch

__all__ = ['Project', 'utils', 'EnsembleTrajectories', 'autocorrelation', 'ensemble_diagnostics', 'ensemble_predictions',
           'ensemble_trajs', 'net_ensemble_trajs', 'pca_eig', 'pca_eig_log_params', 'temperature_ladder',
           'traj_ensemble_quantiles', 'traj_ensemble_stats', 'profile_confidence_intervals', 'profile_likelihood_batch']
