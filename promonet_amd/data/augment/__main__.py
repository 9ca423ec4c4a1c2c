import argparse

import promonet_amd


def parse_args():
    """Parse command-line arguments"""
    parser = argparse.ArgumentParser(description='Perform data augmentation')
    parser.add_argument(
        '--datasets',
        nargs='+',
        default=promonet_amd.DATASETS,
        help='The name of the datasets to augment')
    parser.add_argument(
        '--gpu',
        type=int,
        default=0,
        help='The index of the GPU to run on')
    return parser.parse_args()


promonet_amd.data.augment.datasets(**vars(parse_args()))
