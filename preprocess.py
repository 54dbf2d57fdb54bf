#!/usr/bin/env python
# coding: utf-8
"""Prepare a mesh or a point cloud for training — reference preprocess.py:

    python preprocess.py path/to/mesh.obj path/to/output/folder/ [-s 100000]        -> <name>_t.obj + <name>_pc.ply
    python preprocess.py path/to/cloud.ply path/to/output/folder/ -pc [-s 100000]   -> <name>_t.ply + <name>_pc.ply
    python preprocess.py path/to/dataset/ ignored [-pc]                              every .obj (.ply) below the folder
    python preprocess.py path/to/scan.ply out/ -pc [--remove-outliers]              a raw scan: its normals are estimated on the GPU

A cloud without `nx, ny, nz` gets normals estimated from its --normals-k nearest neighbours and oriented consistently
(`--estimate-normals` forces that for a cloud that has some); `--remove-outliers` first drops the points whose mean distance to their
--nb-neighbors nearest neighbours lies more than --std-ratio standard deviations above the cloud's mean.  Both run on the GPU.

A folder is walked as the reference walks it: files that end in `_t` or `_pc` are outputs and are skipped; a mesh's files go to
`<its folder>/<name>/`, a cloud's files next to it."""
import argparse
import os

from src.preprocess_mesh import preprocessMesh, preprocessPointCloud


def main(argv=None):
    parser = argparse.ArgumentParser(description='Preprocess triangle mesh for training')
    parser.add_argument('input_path', metavar='path/to/mesh', type=str, help='path to input mesh')
    parser.add_argument('output_path', metavar='path/to/output/folder/', type=str, help='path to output point cloud')
    parser.add_argument('-s', '--samples', type=int, default=1e5, help='surface samples')
    parser.add_argument('-pc', '--pointcloud', action='store_true', help='use pointcloud as input w/o need of triangle mesh')
    parser.add_argument('--seed', type=int, default=123, help='seed of the surface samples')
    parser.add_argument('--estimate-normals', action='store_true', help='-pc: estimate the normals even if the cloud has some '
                        '(a cloud without normals always gets them estimated)')
    parser.add_argument('--normals-k', type=int, default=15, help='-pc: neighbours of the normal estimation')
    parser.add_argument('--remove-outliers', action='store_true', help='-pc: statistical outlier removal before anything else')
    parser.add_argument('--nb-neighbors', type=int, default=16, help='-pc: neighbours of the outlier test')
    parser.add_argument('--std-ratio', type=float, default=2.0, help='-pc: standard deviations above the mean a point may lie')
    args = parser.parse_args(argv)

    inputPath, outputPath = args.input_path, args.output_path
    scan = dict(estimate_normals=True if args.estimate_normals else None, normals_k=args.normals_k, remove_outliers=args.remove_outliers,
                nb_neighbors=args.nb_neighbors, std_ratio=args.std_ratio)
    if os.path.isfile(inputPath):
        print('Preparing point cloud...')
        if args.pointcloud:
            preprocessPointCloud(outputPath, inputPath, surfacePoints=args.samples, seed=args.seed, **scan)
        else:
            preprocessMesh(outputPath, inputPath, surfacePoints=args.samples, seed=args.seed)
        return
    ext = '.ply' if args.pointcloud else '.obj'
    for dirpath, dirnames, filenames in os.walk(inputPath):
        for file in sorted(filenames):
            if file[-4:] == ext and file[-6:-4] != '_t' and file[-7:-4] != '_pc':
                print(f'Processing {dirpath[dirpath.rfind("/") + 1:]}...')
                if args.pointcloud:
                    preprocessPointCloud(dirpath, os.path.join(dirpath, file), surfacePoints=args.samples, seed=args.seed, **scan)
                else:
                    preprocessMesh(os.path.join(dirpath, file[:-4]), os.path.join(dirpath, file), surfacePoints=args.samples,
                                   seed=args.seed)


if __name__ == '__main__':
    main()
